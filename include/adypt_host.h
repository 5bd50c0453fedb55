/*
 * adypt_host.h — C-ABI of the host-side pieces either side of the GPU path: the .config scene interface, OBJ/MTL
 * scene loading, the CPU SBVH -> CWBVH8 builder and its .bvh cache, camera matrices, Sobol stream, EXR output.
 * They reproduce what Instance::Initialize (src/Instance.cpp:10-42) strings together in the reference so that the
 * tracer (adypt_hip.h) can run headless from an Adypt .config file.  None of these functions needs a GPU.
 */
#ifndef ADYPT_HOST_H
#define ADYPT_HOST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- InstanceConfig (src/InstanceConfig.hpp:12-48, src/InstanceConfig.cpp:10-192) ------------------------------ */
typedef struct adypt_bvh_params { /* InstanceConfig::BVH; also the 12-byte header field of the .bvh cache */
	int32_t max_spatial_depth;
	float triangle_sah, node_sah;
} adypt_bvh_params;

typedef struct adypt_config {
	int32_t width, height;
	adypt_bvh_params bvh;
	/* InstanceConfig::PT */
	int32_t invocation_size, stack_size, max_bounce, subpixel, tmp_lifetime;
	float ray_tmin, clamp, sun[3];
	/* InstanceConfig::Cam */
	float speed, mouse_sensitive, fov, yaw, pitch, position[3];
	char obj_filename[1024], bvh_filename[1024];
} adypt_config;

void adypt_config_default(adypt_config *cfg);                       /* InstanceConfig::SetDefault */
int adypt_config_load(const char *path, adypt_config *cfg);         /* InstanceConfig::LoadFromFile (strict: all keys, typed) */
int adypt_config_parse(const char *json_text, adypt_config *cfg);
/* InstanceConfig::GetJson: writes at most cap bytes incl. NUL, returns the needed size */
size_t adypt_config_json(const adypt_config *cfg, char *buf, size_t cap);
int adypt_config_save(const char *path, const adypt_config *cfg);   /* InstanceConfig::SaveToFile */
const char *adypt_host_last_error(void);

/* Camera::Control (src/Tracer/Camera.cpp:25-59) without the window: the key / mouse state GLFW and ImGui would report is
 * passed in.  keys: ADYPT_KEY_* bits held this frame; mouse_dx/dy: cursor movement in pixels while the left button is
 * held (0 otherwise); frame_seconds: fps.GetDelta().  Same arithmetic: move = frame_seconds * speed along yaw (+90 / -90 /
 * 180 degrees for A / D / S), space / shift move along y, yaw -= dx * sensitivity (mod 360), pitch -= dy * sensitivity
 * clamped to [-90, 90]. */
enum { ADYPT_KEY_W = 1, ADYPT_KEY_A = 2, ADYPT_KEY_S = 4, ADYPT_KEY_D = 8, ADYPT_KEY_SPACE = 16, ADYPT_KEY_LEFT_SHIFT = 32 };
void adypt_camera_control(adypt_config *cfg, uint32_t keys, float mouse_dx, float mouse_dy, float frame_seconds);

/* ---- Scene (src/Util/Scene.cpp:9-136) + material/texture conversion (src/Tracer/OglScene.cpp:12-91) ------------- */
typedef struct adypt_scene adypt_scene;
int adypt_scene_load(const char *obj_path, adypt_scene **out);      /* Scene::LoadFromFile + init_materials */
void adypt_scene_free(adypt_scene *s);
int64_t adypt_scene_triangles(const adypt_scene *s, const void **tris);   /* 100-byte records, OBJ order */
int64_t adypt_scene_materials(const adypt_scene *s, const void **mats);   /* 64-byte GPUMaterial records */
int32_t adypt_scene_textures(const adypt_scene *s, const void **tex /* adypt_texture[] */);
void adypt_scene_aabb(const adypt_scene *s, float lo[3], float hi[3]);
/* "" or one line per diffuse texture that could not be decoded: like the reference after a failed stbi_load
 * (src/Tracer/OglScene.cpp:12-43) the scene still loads and the material renders with Kd = 0, but the loss is reported
 * (this loader reads PNM, PNG, BMP, TGA and JPEG with stb_image's pixels; stb_image also reads GIF, PSD, HDR, PIC and 16-bit BMP) */
const char *adypt_scene_warnings(const adypt_scene *s);
/* wrap caller-provided triangles (no OBJ): used for huge procedural scenes */
int adypt_scene_from_arrays(const void *tris, int64_t n_tris, const void *mats, int64_t n_mats, adypt_scene **out);

/* ---- BVH (src/BVH/SBVHBuilder.*, WideBVHBuilder.*, WideBVH.*) ---------------------------------------------------- */
typedef struct adypt_bvh adypt_bvh;
typedef struct adypt_build_info {
	int64_t sbvh_nodes, refs, wide_nodes;
	double sbvh_ms, wide_ms;
} adypt_build_info;
/* Worker threads of adypt_bvh_build (the reference's SBVHBuilder is single-threaded,
 * src/BVH/SBVHBuilder.cpp:49-71).  0 = automatic: $ADYPT_BUILD_THREADS, else the cores the process may use.  The
 * node and index arrays do not depend on the thread count. */
int adypt_host_set_threads(int n);
int adypt_host_get_threads(void);
/* Self-test of the multi-threaded sort the parallel build uses for its largest nodes (csrc/host/exact_sort.hpp): it
 * must return the very permutation std::sort returns (ties between the halves of a split triangle make the
 * permutation part of the node array).  pattern 0 random, 1 heavy ties, 2 sorted, 3 reversed, 4 all equal,
 * 5 quicksort killer (reaches the heap-sort fallback).  Returns 0 when both sorts agree byte for byte. */
int adypt_host_selftest_sort(int64_t n, uint32_t seed, int pattern, int threads, int64_t min_task);
/* SBVHBuilder{cfg,&sbvh,scene}.Run(); WideBVHBuilder{cfg,&wbvh,sbvh}.Run(); (src/Instance.cpp:24-26).  ADYPT_E_INVALID, like every builder below and
 * like the device's, for a scene whose SAH costs are not finite numbers below FLT_MAX (node areas past about 2^127: vertices that are NaN, infinite or
 * huge): the sweep then has no split to take and the collapse no cut. */
int adypt_bvh_build(const adypt_scene *s, const adypt_bvh_params *p, adypt_bvh **out, adypt_build_info *info);
/* A CWBVH8 from a linear BVH: Morton keys of the centroids, a sort, Karras's radix tree, the collapse above, and boxes by the rule of adypt_bvh_refit.
 * The definition is csrc/device/lbvh.hpp, which the device builder (adypt_hip.h, adypt_rebuild_bvh) compiles too: both give the same bytes.  No
 * spatial splits (max_spatial_depth is ignored), so there is one reference per triangle; triangle_sah and node_sah steer the collapse and must be
 * positive finite numbers.  info: sbvh_nodes = the binary nodes (2 n - 1), sbvh_ms = keys, sort and tree, wide_ms = collapse and boxes.  Faster to
 * build and slower to trace than adypt_bvh_build's tree (Rebuilding on the GPU). */
int adypt_bvh_build_linear(const adypt_scene *s, const adypt_bvh_params *p, adypt_bvh **out, adypt_build_info *info);
/* the sorted keys adypt_bvh_build_linear makes of n_tris 100-byte triangle records: Morton code << 32 | triangle index, ascending (for tests and tools) */
int adypt_lbvh_keys(const void *tris, int64_t n_tris, uint64_t *out);
/* A CWBVH8 from the same keys and the same sort, but with the binary tree built bottom up by PLOC (parallel locally-ordered clustering): in rounds,
 * every cluster looks `radius` clusters to either side in Morton order for the one whose union with it has the smallest area, and two clusters that
 * choose each other merge.  The definition is csrc/device/ploc.hpp, which the device builder (adypt_hip.h, adypt_rebuild_bvh_ploc) compiles too: both
 * give the same bytes.  Collapse, layout and boxes are adypt_bvh_build_linear's, and so are the arguments and `info`; radius is in [1, 32], 8 is the
 * default of the callers.  The tree does not depend on adypt_host_set_threads.  ADYPT_E_INVALID also for a triangle whose box has no finite area and
 * for a round that merges nothing (areas that overflow).  A tighter tree than the linear one on meshes (Rebuilding on the GPU). */
int adypt_bvh_build_ploc(const adypt_scene *s, const adypt_bvh_params *p, int radius, adypt_bvh **out, adypt_build_info *info);
/* the binary tree adypt_bvh_build_ploc makes of n_tris 100-byte triangle records, in the node ids of csrc/device/lbvh.hpp: left[i] and right[i] are
 * the children of inner node i (n_tris - 1 entries each; the root is 0; the leaf of sorted position j is n_tris - 1 + j).  For tests and tools. */
int adypt_ploc_tree(const void *tris, int64_t n_tris, int radius, int32_t *left, int32_t *right);
/* adypt_bvh_build_ploc with large triangles split into several references first (early split clipping; the definition is csrc/device/presplit.hpp,
 * which the device builder, adypt_rebuild_bvh_ploc_split, compiles too: both give the same bytes).  A triangle whose box is large against the scene's
 * is cut at the middle of its box's longest axis, again and again (at most 6 times in a row), and every piece becomes a reference with the clipped
 * piece's box; the tree holds at most n + floor(split_budget * n) references, split_budget in [0, 1] (else ADYPT_E_INVALID; NaN too).  The level of
 * detail is the finest of 24 (areas of S * 2^-level, S the scene box's area) that stays inside the budget.  tri_indices names a split triangle once per
 * reference; the leaf slots bound the references' boxes (adypt_bvh_ref_boxes), not the whole triangles, which is the gain: a long thin triangle no
 * longer puts a box the size of a room into a leaf.  Budget 0, or a budget under which nothing is split, gives adypt_bvh_build_ploc's tree to the
 * byte.  Like a tree with spatial splits, a split tree should be rebuilt for a new pose, not refitted: adypt_bvh_refit bounds whole triangles.
 * info->refs: the references.  The tree does not depend on adypt_host_set_threads. */
int adypt_bvh_build_ploc_split(const adypt_scene *s, const adypt_bvh_params *p, int radius, double split_budget, adypt_bvh **out, adypt_build_info *info);
/* the boxes of that tree's references in the order of tri_indices, 6 floats each (lo xyz, hi xyz); returns their number — 0, and *boxes = NULL, for a
 * tree that has none (every other builder's, and a split build that split nothing) */
int64_t adypt_bvh_ref_boxes(const adypt_bvh *b, const float **boxes);
/* the bare reference list adypt_bvh_build_ploc_split starts from, for n_tris 100-byte records, in reference order (triangles in index order, the pieces
 * of one depth first, low half first): *level the chosen level or -1, ref_tri[r] the triangle, ref_box + 6 r its box.  Returns the number of references,
 * and writes the arrays only when that is <= capacity (call with capacity 0 to ask); negative: an ADYPT_E_* code.  For tests and tools. */
int64_t adypt_presplit_refs(const void *tris, int64_t n_tris, double split_budget, int64_t capacity, int32_t *level, int32_t *ref_tri, float *ref_box);
int adypt_bvh_load(const char *path, const adypt_bvh_params *expected, adypt_bvh **out);  /* WideBVH::LoadFromFile */
int adypt_bvh_save(const adypt_bvh *b, const char *path, const adypt_bvh_params *p);       /* WideBVH::SaveToFile */
void adypt_bvh_free(adypt_bvh *b);
int64_t adypt_bvh_nodes(const adypt_bvh *b, const void **nodes);          /* 80-byte records */
int64_t adypt_bvh_tri_indices(const adypt_bvh *b, const int32_t **idx);
/* Moved geometry without a rebuild: recomputes, in place, the boxes of `nodes` (p, the exponent bytes and the quantised bytes of every occupied slot)
 * from the triangles as they are now.  The topology and the reference order stay, so tri_indices and the triangle count must be the tree's.  The rule
 * is csrc/device/refit.hpp (the device path, adypt_update_triangles, compiles the same text); the Woop array is adypt_woop_matrices of the moved
 * triangles.  A leaf bounds its whole triangles, so a tree built with spatial splits gets larger boxes than the builder's clipped ones: correct, but
 * slower to traverse (Moving geometry).  ADYPT_E_INVALID — nothing is written — for arrays that are not one tree: a child index or a
 * reference range out of range, a node reached twice or not at all, a triangle index out of range. */
int adypt_bvh_refit(void *nodes, int64_t n_nodes, const int32_t *tri_indices, int64_t n_refs, const void *triangles, int64_t n_tris);
/* The SAH cost of a tree as the traversal sees it, from the quantised child boxes of the 80-byte nodes alone: every occupied slot's area over the area
 * of the root (the union of node 0's slots), as an integer q = the ratio * 2^30 cut off; inner_q is the sum of q over the slots that hold a child
 * node, leaf_q the sum of q * (the slot's references) over the leaf slots, and cost = node_sah * (1 + inner_q / 2^30) + triangle_sah * leaf_q / 2^30 in
 * binary64: the node visits and triangle tests a random ray through the root is expected to make, priced.  The rule is csrc/device/tree_cost.hpp (the
 * device path, adypt_get_tree_cost, compiles the same text and gives the same integers).  What it is for: a refitted tree's cost over the cost it had
 * when it was built says how much slower the refitted tree traverses (Moving geometry; adypt_update_triangles_auto).  params: NULL for the
 * defaults (triangleSAH 0.3, nodeSAH 1); max_spatial_depth is ignored.  ADYPT_E_INVALID — *out is not written — for no nodes or more than 2^26, SAH
 * costs that are not positive finite numbers, a root without a positive finite area (all triangles at one point) and a slot of four times the root's
 * area or more. */
#ifndef ADYPT_TREE_COST_DEFINED
#define ADYPT_TREE_COST_DEFINED
typedef struct adypt_tree_cost {
	double cost;
	uint64_t inner_q, leaf_q;
	int64_t n_nodes;
} adypt_tree_cost;
#endif
int adypt_bvh_cost(const void *nodes, int64_t n_nodes, const adypt_bvh_params *params, adypt_tree_cost *out);

/* ---- small restated host functions ---------------------------------------------------------------------------- */
/* One 80-byte CWBVH8 node decoded into the 264-byte root card of the device's k_path (csrc/device/root_card.hpp: the definition, which the device
 * compiles too; adypt_read_root_card of adypt_hip.h reads a context's).  allow = 0: the card's `enabled` word stays 0 whatever the node holds. */
void adypt_decode_root_card(const void *node, int allow, void *card_out);
/* OglScene::init_triangles (src/Tracer/OglScene.cpp:93-116): out = 12 floats per reference */
void adypt_woop_matrices(const void *tris, const int32_t *tri_indices, int64_t n_refs, float *out);
/* The device triangle records of `n_tris` 100-byte Triangles (src/Util/Shape.hpp:70-74): records_out = n_tris x 128 bytes — floats 0..17 positions and
 * normals, word 18 the material id, word 19 the class word (1 where the material runs the glossy lobe or the dielectric branch, 0 otherwise and for an
 * id outside [0, n_mats)), floats 20..25 the texture coordinates, the rest zero; classes_out = one shading-class byte per triangle (1..6; 5 for an id
 * outside [0, n_mats)).  Either may be NULL.  materials: n_mats 64-byte GPUMaterial.  The definition is csrc/device/tri_record.hpp, which the device
 * (adypt_set_triangles of adypt_hip.h) compiles too: both give the same bytes.  ADYPT_E_INVALID for a null array that is needed or a negative count. */
int adypt_pack_triangles(const void *triangles, int64_t n_tris, const void *materials, int64_t n_mats, int32_t n_textures, void *records_out, uint8_t *classes_out);
/* The device's material table and texture arena of a scene: records_out = n_mats x 80 bytes — a material's 64 bytes, then (texel offset, w, h, 0) of its
 * diffuse texture where 0 <= dtex < n_textures, else 16 zero bytes; texels_out = the arena's words — texture after texture, back to back, each h rows of
 * w + 1 words r | g << 8 | b << 16 | 0xff000000, a row's last word a copy of its first; desc_out = n_textures x (offset, w, h, 0).  Any output may be
 * NULL.  textures: n_textures adypt_texture (adypt_hip.h).  Returns the arena's length in words (below 2^31), so a first call with NULL outputs gives
 * the size of texels_out.  The definition is csrc/device/appearance.hpp, which the device (adypt_set_materials, adypt_update_texture of adypt_hip.h)
 * compiles too: both give the same bytes.  ADYPT_E_INVALID — nothing is written — for a null array that is needed, a negative count, a texture
 * without pixels or 2^31 texels and more. */
int64_t adypt_pack_appearance(const void *materials, int64_t n_mats, const void *textures /* adypt_texture[] */, int32_t n_textures, void *records_out, uint32_t *texels_out,
                              int32_t *desc_out);
/* `n_tris` 100-byte Triangles posed by row-major 3x4 matrices (n_matrices x 12 floats, n_matrices in [1, 65536]): positions through the matrix, normals
 * through its cofactor matrix and normalised again, texture coordinates and material id as they are; triangles_out = n_tris x 100 bytes, which may be
 * triangles_in.  Either parts (one index per triangle) or joints and weights (n_tris x 12 each: vertex v's four slots at 4 v; a slot of weight 0 is
 * skipped, its index never read) is given, the other NULL.  The definition is csrc/device/pose.hpp, which the device (adypt_pose of adypt_hip.h)
 * compiles too: both give the same bits.  ADYPT_E_INVALID — nothing is written — for what adypt_bind_parts / adypt_bind_skin / adypt_pose refuse. */
int adypt_pose_triangles(const void *triangles_in, int64_t n_tris, const int32_t *parts_or_null, const uint16_t *joints_or_null, const float *weights_or_null, const float *matrices,
                         int32_t n_matrices, void *triangles_out);
/* adypt_pose_triangles with a morph layer in front of the matrices (csrc/device/pose.hpp: rest pose -> morph -> vertex matrix): n_entries sparse
 * entries in any order, entry e being (triangle_of_entry[e], target_of_entry[e], deltas[18 e .. 18 e + 17]) — the deltas of p0 p1 p2 n0 n1 n2 — and
 * n_targets weights, finite and of any sign.  A triangle's entries are applied in ascending target index, acc = acc + w * d per word, an entry of
 * weight 0 skipped: all weights 0 give adypt_pose_triangles' bytes.  The whole pipeline of adypt_bind_morph + adypt_pose_morph (adypt_hip.h) on the
 * host, bit for bit.  ADYPT_E_INVALID — nothing is written — for what those two refuse. */
int adypt_pose_triangles_morph(const void *triangles_in, int64_t n_tris, const int32_t *parts_or_null, const uint16_t *joints_or_null, const float *weights_or_null,
                               const float *matrices, int32_t n_matrices, const int32_t *triangle_of_entry, const int32_t *target_of_entry, const float *deltas /* n_entries x 18 */,
                               int64_t n_entries, const float *morph_weights /* n_targets */, int32_t n_targets, void *triangles_out);
/* A dense target mesh as sparse morph entries: the triangles whose words 0..17 (positions, normals) differ in any bit between two arrays of n_tris
 * 100-byte Triangles, in ascending order into triangle_out, and d = target - rest, one binary32 subtraction per word, into deltas_out (18 floats per
 * listed triangle).  Returns their number; either output may be NULL (both NULL: the size only, at most n_tris).  Weight 1 then gives
 * rest + (target - rest), which is the target only up to one rounding.  ADYPT_E_INVALID (negative) for a null input or a negative count. */
int64_t adypt_morph_diff(const void *rest, const void *target, int64_t n_tris, int32_t *triangle_out, float *deltas_out);
/* The smooth normals of an indexed mesh (csrc/device/mesh.hpp, which the device — adypt_pose_vertices of adypt_hip.h without normals — compiles too:
 * both give the same bits): indices n_tris x 3, each in [0, n_vertices); positions and normals_out n_vertices x 3 floats.  A vertex's normal is the
 * sum of its triangles' area-weighted face vectors in ascending 3 t + c, divided by its length where that is a positive finite number; a vertex that
 * no triangle names gets +0.  ADYPT_E_INVALID — nothing is written — for a null array, a negative n_tris, n_vertices outside [1, 2^31 - 1], an index
 * out of range or a position that is not finite. */
int adypt_mesh_normals(const int32_t *indices, int64_t n_tris, int64_t n_vertices, const float *positions, float *normals_out);
/* `n_tris` 100-byte Triangles with words 0..17 replaced by the mesh: corner c of triangle t takes positions[indices[3 t + c]] and that vertex's
 * normal — given (used as given; finite), or with normals_or_null NULL computed as adypt_mesh_normals does.  Texture coordinates and material ids
 * stay.  The host's side of adypt_bind_mesh + adypt_pose_vertices.  ADYPT_E_INVALID — nothing is written — for what those two refuse. */
int adypt_mesh_triangles(const void *triangles_in, int64_t n_tris, const int32_t *indices, int64_t n_vertices, const float *positions, const float *normals_or_null,
                         void *triangles_out);
/* The index buffer of a triangle soup.  A vertex is the 24 bytes of a corner's position and normal, compared as bits; vertices are numbered in order
 * of first appearance over corners in ascending 3 t + c, so corners at one position with different normals (a crease) stay different vertices.
 * Returns n_vertices; any output may be NULL (all NULL: the size only, at most 3 n_tris): indices_out n_tris x 3, positions_out and normals_out
 * n_vertices x 3 floats.  adypt_mesh_triangles of the three arrays has the soup's bytes.  ADYPT_E_INVALID (negative) for a null input or 3 n_tris
 * outside [0, 2^31 - 1]. */
int64_t adypt_weld_triangles(const void *triangles, int64_t n_tris, int32_t *indices_out, float *positions_out, float *normals_out);
/* Camera::GetView/GetProjection + the inverses of SetCamera (src/Tracer/Camera.cpp:13-23, OglPathTracer.cpp:27-32) */
void adypt_camera_matrices(float fov, float yaw, float pitch, int width, int height, float inv_proj[16], float inv_view[16]);
/* Sobol::Next (src/Util/Sobol.cpp:16-21): points of frames [first, first+n), dim <= 64; out = n*dim floats */
int adypt_sobol_points(int dim, int first, int n, float *out);
/* RG8 shift image bytes from mt19937(seed) (src/Tracer/OglPathTracer.cpp:156-162): width*height*2 bytes */
void adypt_shift_bytes(uint32_t seed, int width, int height, uint8_t *out);
/* SaveEXR(rgb, W, H, 3, fp16, path) as OglPathTracer::SaveResult calls it (OglPathTracer.cpp:207): scanline,
 * ZIP, channels B,G,R, HALF or FLOAT */
int adypt_save_exr(const char *path, const float *rgb, int width, int height, int save_as_fp16);
/* 8-bit RGBA (adypt_read_display) -> PNG: the headless stand-in for the reference's window */
int adypt_save_png(const char *path, const uint8_t *rgba8, int width, int height);
/* minimal reader of the files adypt_save_exr writes (round-trip tests / tools) */
/* stbi_load(filename, &w, &h, &channels, 3) as OglScene::load_texture calls it (src/Tracer/OglScene.cpp:26-34): tightly packed RGB8, row 0
 * = top.  PNM, PNG (all depths, Adam7), BMP, TGA, JPEG (baseline / progressive; stb_image's own IDCT, up-sampling and colour arithmetic),
 * all pinned to the reference's stb_image by tests/golden/images.  *rgb is released with adypt_free. */
int adypt_load_image_rgb8(const char *path, uint8_t **rgb, int32_t *width, int32_t *height);
int adypt_load_exr(const char *path, float **rgb, int *width, int *height);
void adypt_free(void *p);

#ifdef __cplusplus
}
#endif
#endif /* ADYPT_HOST_H */
