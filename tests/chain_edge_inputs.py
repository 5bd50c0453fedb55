"""The hand-made edge inputs of k_chain_start and k_chain_step, named once (not a test module): a scene of a few triangles and materials no traversal
ever sees — every illum, a texture, material ids and hit words outside their tables, ior 0 and NaN, zero normals — block lists and followed-pixel
patterns for the start, and queues of rays of every kind for the step, with the truths composed from tests/specular_truth.py (start, step) and
tests/virtual_truth.py (the lengths and the virtual point).  Every entry's `reach` is computed from its inputs or from the truth, never from the
device's output.  tests/test_specular_definition.py and tests/test_virtual_definition.py run the entries through the header on the CPU,
tests/test_gpu_chain_probes.py through the kernels."""
import numpy as np

from oracle import oracle_py as O
from tests import specular_truth as S
from tests import tri_record_truth as TR
from tests import virtual_truth as V
from tests.probe import UNWRITTEN, device_materials

F, U32, I32 = np.float32, np.uint32, np.int32
MARK = F(55.0)      # what the .w of a hit, and a virtual point, hold going in: a word the kernels must leave where they write nothing
INT_MAX = 2 ** 31 - 1
ORIGIN = np.array([1.0, 2.0, 3.0], np.float32)
TMIN = F(0.001)
SENTINEL = np.array([UNWRITTEN], U32).view(F)[0]


def as_float(words):
    return np.asarray(words, I32).view(F)


def as_word(floats):
    return np.ascontiguousarray(floats, dtype=F).view(I32)


# ---- the scene ----
class Scene:
    """what specular_truth's materials_of, tri_words and textured_kd read of an oracle scene, and the device's tables of the same"""

    def __init__(self, triangles, materials, texture):
        self.triangles, self.materials, self.textures = triangles, materials, [texture]
        self.device = (TR.pack(triangles, materials, 1)[0], device_materials(materials, texture), texture)


# materials 0..8: illum 0..8; then a textured diffuse one, glass of ior 0 and of ior NaN, a mirror that names the texture (never fetched)
M_TEXTURED, M_IOR_0, M_IOR_NAN, M_MIRROR_TEXTURED, N_MATS = 9, 10, 11, 12, 13
# triangles 0..12: one per material; then material ids -1 and N_MATS, zero normals on a diffuse and on a mirror material
T_MATID_M1, T_MATID_N, T_ZERO_N_DIFFUSE, T_ZERO_N_MIRROR, N_TRIS = 13, 14, 15, 16, 17
HIT_WORDS_ESCAPED = [-1, -2, -7, N_TRIS, INT_MAX]


def scene():
    rs = np.random.RandomState(301)
    m = np.zeros(N_MATS, O.MAT_DT)
    m["dtex"], m["etex"], m["stex"] = -1, -1, -1
    m["kd"], m["ks"] = rs.uniform(0.2, 0.9, (N_MATS, 3)), rs.uniform(0.5, 1.0, (N_MATS, 3))
    m["illum"][:9] = np.arange(9)
    m["illum"][M_TEXTURED], m["dtex"][M_TEXTURED] = 1, 0
    m["illum"][M_IOR_0], m["illum"][M_IOR_NAN] = 7, 6
    m["illum"][M_MIRROR_TEXTURED], m["dtex"][M_MIRROR_TEXTURED] = 3, 0
    m["shininess"], m["dissolve"], m["ior"] = 10.0, 1.0, 1.5
    m["ior"][M_IOR_0], m["ior"][M_IOR_NAN] = 0.0, np.nan
    t = np.zeros(N_TRIS, O.TRI_DT)
    t["p"], t["n"], t["tc"] = rs.uniform(-3, 3, (N_TRIS, 3, 3)), rs.normal(0, 1, (N_TRIS, 3, 3)), rs.uniform(-1, 2, (N_TRIS, 3, 2))
    t["n"] += t["n"][:, :1] * 3  # (the three normals of a triangle lie within a right angle of each other: none interpolates to zero by accident)
    t["matid"] = np.arange(N_TRIS)
    t["matid"][T_MATID_M1], t["matid"][T_MATID_N], t["matid"][T_ZERO_N_DIFFUSE], t["matid"][T_ZERO_N_MIRROR] = -1, N_MATS, 1, 3
    t["n"][T_ZERO_N_DIFFUSE], t["n"][T_ZERO_N_MIRROR] = 0, 0
    t["tc"][M_TEXTURED] = [[1, 0], [0, 1], [0, 0]]  # s = u, t = v
    texture = rs.randint(0, 256, (3, 4, 3)).astype(np.uint8)
    return Scene(t, m, texture)


# ---- k_chain_start ----
# a pixel's kind: (hit word, what is done to its guides).  FOLLOWED kinds go on whatever K >= 1 is; the others never do
FOLLOWED = [(3, None), (4, None), (5, None), (6, None), (7, None), (M_MIRROR_TEXTURED, None)]
NOT_FOLLOWED = [(w, None) for w in HIT_WORDS_ESCAPED] + [(T_MATID_M1, None), (T_MATID_N, None), (0, None), (1, None), (2, None), (8, None), (M_TEXTURED, None), (3, "at-origin"),
                                                         (7, "at-origin"), (3, "nan-normal"), (6, "nan-normal")]
EITHER = [(M_IOR_0, None), (M_IOR_NAN, None)]  # the truth says
# (blocks 0 and 1 lie wholly inside 70 x 40, block 5 is its corner of 6 x 8 pixels: the first and the last block of every list are whole, so that local pixels
# 0, 63, 64 and the last one are pixels of the picture; a start writes no picture, so a block may repeat)
START_PICTURES = {"70x40": (70, 40, {1: [0], 2: [1, 0], 3: [0, 5, 1]}), "1x1": (1, 1, {1: [0], 2: [0, 0], 3: [0, 0, 0]})}
START_SEGMENTS = [1, 3, 8]
START_PATTERNS = ["none", "local-0", "local-63", "local-64", "last", "every-other-lane", "one-workgroup", "all", "mixed-K1", "mixed-K8"]


def inside(blocks, w, h):
    """(n_px,) bool: the local pixel lies in the picture (the block-major layout is denoise_edge_inputs.block_major's)"""
    from tests.denoise_edge_inputs import block_major
    return block_major(np.ones((h, w, 4), F), np.asarray(blocks), w, h)[:, 0] != 0


def start_case(picture, n_blocks, pattern):
    w, h, lists = START_PICTURES[picture]
    blocks = np.array(lists[n_blocks], I32)
    n_px = len(blocks) * 1024
    rs = np.random.RandomState(302 + n_px)
    L = np.arange(n_px)
    want = {"none": L < 0, "local-0": L == 0, "local-63": L == 63, "local-64": L == 64, "last": L == n_px - 1, "every-other-lane": L % 2 == 1, "one-workgroup": L // 256 == n_px // 256 - 3,  # (of the last block)
            "all": L >= 0}.get(pattern)
    kinds = NOT_FOLLOWED if want is not None else NOT_FOLLOWED + FOLLOWED + EITHER
    kind = L % len(kinds)
    if want is not None:
        kinds = kinds + FOLLOWED
        kind = np.where(want, len(NOT_FOLLOWED) + L % len(FOLLOWED), kind)
    word = np.array([k[0] for k in kinds], I32)[kind]
    how = np.array([k[1] or "" for k in kinds])[kind]
    normal = rs.normal(0, 1, (n_px, 3)).astype(F)
    normal /= np.sqrt((normal * normal).sum(-1, keepdims=True)).astype(F)
    position = rs.uniform(-3, 3, (n_px, 3)).astype(F)
    position[how == "at-origin"] = ORIGIN
    normal[how == "nan-normal", 1] = np.nan
    hits = np.concatenate([as_float(word)[:, None], rs.uniform(0, 0.5, (n_px, 2)).astype(F), np.full((n_px, 1), MARK, F)], 1)
    g = dict(albedo=np.concatenate([rs.uniform(0, 1, (n_px, 3)).astype(F), np.ones((n_px, 1), F)], 1), normal=np.concatenate([normal, np.ones((n_px, 1), F)], 1),
             position=np.concatenate([position, np.ones((n_px, 1), F)], 1), hits=hits)
    return dict(w=w, h=h, blocks=blocks, n_px=n_px, word=word, how=how, want=want, K=1 if pattern == "mixed-K1" else 8, inside=inside(blocks, w, h), **g)


def start_truth(sc, case, unfold, ops=None, lengths=None):
    """What k_chain_start<unfold> leaves: dict(go (n_px,) bool; hits_w (n_px,): the .w of every hit; state (n_px, 2, 4) with the sentinel where the pixel
    is not followed; o, d (n_px, 4): the ray of a followed pixel)"""
    n_px, ins = case["n_px"], case["inside"]
    at = np.flatnonzero(ins)
    r = S.start(sc, case["word"][at], case["normal"][at, :3], case["position"][at, :3], ORIGIN, case["K"], ops=ops, unfold=(lengths or V.NumpyUnfold()) if unfold else None)
    go = np.zeros(n_px, bool)
    go[at] = r["go"]
    hits_w = np.full(n_px, MARK, F)
    hits_w[at] = np.where(r["go"], MARK, r["cls"])
    state = np.full((n_px, 2, 4), SENTINEL, F)
    o, d = np.zeros((n_px, 4), F), np.zeros((n_px, 4), F)
    f = at[r["go"]]
    state[f, 0, :3], state[f, 0, 3], state[f, 1, :3], state[f, 1, 3] = r["T"][r["go"]], as_float(np.zeros(len(f), I32)), r["d"][r["go"]], r["length"][r["go"]]
    o[f, :3], o[f, 3], d[f, :3], d[f, 3] = case["position"][f, :3], TMIN, r["d"][r["go"]], as_float(f)
    return dict(go=go, hits_w=hits_w, state=state, o=o, d=d)


def start_reach(case, t):
    go, ins = t["go"], case["inside"]
    if case["want"] is not None:
        return bool(np.array_equal(go, case["want"] & ins) and (go.any() == case["want"].any() or case["w"] == 1))
    seen = set(zip(case["word"][ins].tolist(), case["how"][ins].tolist()))
    every = len(seen) == len(NOT_FOLLOWED + FOLLOWED + EITHER) or case["w"] == 1
    followed = all(go[ins & (case["word"] == k[0]) & (case["how"] == "")].all() for k in FOLLOWED)
    never = all(not go[ins & (case["word"] == k[0]) & (case["how"] == (k[1] or ""))].any() for k in NOT_FOLLOWED)
    return bool(every and followed and never and not go[~ins].any())


# the one overflow: a single wave of 64 followed pixels, seg_cap 40, two segments
def overflow_case():
    case = start_case("70x40", 1, "none")
    lanes = np.arange(64)
    case["word"][lanes] = np.array([k[0] for k in FOLLOWED], I32)[lanes % len(FOLLOWED)]
    case["how"][lanes] = ""
    case["hits"][:, 0] = as_float(case["word"])
    case["normal"][:64, :3] = np.array([0.6, 0.0, 0.8], F)
    case["position"][:64, :3] = np.random.RandomState(7).uniform(-3, 3, (64, 3)).astype(F)
    case["want"] = np.arange(case["n_px"]) < 64
    return case


# ---- k_chain_step ----
STEP_N_PX, STEP_SEGMENTS, STEP_SEG_CAP, STEP_K = 2048, 3, 300, 8
STEP_COUNTS = {"0-1-63": [0, 1, 63], "65-257-above-cap": [65, 257, 400]}
BAD_L = [-1, STEP_N_PX, INT_MAX]
TEX_U, TEX_V = [0.0, 0.125, 0.25, 0.5, 0.875, 0.95, 1.0], [0.0, 1.0 / 6, 1.0 / 3, 0.9]  # texel centres, texel edges and the wrap column of the 4 x 3 texture
# a ray's kind: (name, hit word, u, v): None = random barycentrics
RAY_KINDS = ([("escaped", w, None, None) for w in (-1, -2, N_TRIS)] + [("diffuse", 1, None, None), ("illum-0", 0, None, None), ("illum-2", 2, None, None), ("illum-8", 8, None, None)]
             + [("textured", M_TEXTURED, u, v) for u in TEX_U for v in TEX_V] + [("bad-material", T_MATID_M1, None, None), ("bad-material", T_MATID_N, None, None)]
             + [("mirror", w, None, None) for w in (3, 4, 5, M_MIRROR_TEXTURED)] * 2 + [("glass", w, None, None) for w in (6, 7)] * 6 + [("ior-0", M_IOR_0, None, None)] * 2
             + [("ior-nan", M_IOR_NAN, None, None), ("zero-normal", T_ZERO_N_DIFFUSE, None, None), ("zero-normal", T_ZERO_N_MIRROR, None, None), ("nan-u", 1, np.nan, None),
                ("nan-u", 3, np.nan, None)])


def step_case(name):
    counts = np.array(STEP_COUNTS[name], U32)
    rs = np.random.RandomState(303 + int(counts.sum()))
    slots = STEP_SEGMENTS * STEP_SEG_CAP
    u = lambda lo, hi, *s: rs.uniform(lo, hi, size=s).astype(F)  # noqa: E731
    unit = lambda n: (lambda v: (v / np.sqrt((v * v).sum(-1, keepdims=True))).astype(F))(rs.normal(0, 1, (n, 3)))  # noqa: E731
    # every slot holds a ray of a pixel of its own, the slots past a segment's count too: a kernel that consumed one would end or move that pixel
    pixel = rs.permutation(STEP_N_PX)[:slots].astype(I32)
    kind = (np.arange(slots) * 7) % len(RAY_KINDS)  # (7 and the number of kinds share no factor: consecutive slots differ, every kind comes round)
    assert np.gcd(7, len(RAY_KINDS)) == 1
    name_of = np.array([k[0] for k in RAY_KINDS])[kind]
    tri = np.array([k[1] for k in RAY_KINDS], I32)[kind]
    bu, bv = u(0.05, 0.45, slots), u(0.05, 0.45, slots)
    for i, k in enumerate(RAY_KINDS):
        if k[2] is not None:
            bu[kind == i] = k[2]
        if k[3] is not None:
            bv[kind == i] = k[3]
    live = (np.arange(slots) % STEP_SEG_CAP) < np.repeat(np.minimum(counts, STEP_SEG_CAP), STEP_SEG_CAP)
    word = pixel.copy()
    if live.sum() > 100:
        at = np.flatnonzero(live)[5::len(np.flatnonzero(live)) // 7][:6]
        word[at] = np.array(BAD_L * 2, I32)  # pixel words that are no pixel, among valid ones
    length_in = (np.arange(slots) // len(RAY_KINDS) + np.arange(slots)) % STEP_K  # the state's length going in: 0 .. K - 1 for every kind
    len_in = u(0.5, 20, slots)
    ended = np.flatnonzero(live & np.isin(name_of, ("diffuse", "textured", "illum-2")))
    if len(ended) > 8:
        len_in[ended[1]], len_in[ended[3]], len_in[ended[5]] = np.inf, np.nan, F(3.2e38)  # (the last: finite, and longer than a valid length may be)
    state = np.zeros((STEP_N_PX, 2, 4), F)
    state[:, 0, :3], state[:, 1, :3], state[:, 1, 3] = u(0.2, 1, STEP_N_PX, 3), unit(STEP_N_PX), u(0.5, 20, STEP_N_PX)
    state[:, 0, 3] = as_float(np.zeros(STEP_N_PX, I32))
    state[pixel, 0, 3], state[pixel, 1, 3] = as_float(length_in.astype(I32)), len_in
    q = dict(o=np.concatenate([u(-3, 3, slots, 3), np.full((slots, 1), TMIN, F)], 1), d=np.concatenate([state[pixel, 1, :3], as_float(word)[:, None]], 1),
             hit=np.stack([as_float(tri), bu, bv, u(0.1, 9, slots)], 1), count=counts)
    q = {k: (v.reshape(STEP_SEGMENTS, STEP_SEG_CAP, 4) if k != "count" else v) for k, v in q.items()}
    g = dict(albedo=np.concatenate([u(0, 1, STEP_N_PX, 3), np.ones((STEP_N_PX, 1), F)], 1), normal=np.concatenate([unit(STEP_N_PX), np.ones((STEP_N_PX, 1), F)], 1),
             position=np.concatenate([u(-3, 3, STEP_N_PX, 3), np.ones((STEP_N_PX, 1), F)], 1),
             hits=np.concatenate([as_float(rs.randint(0, N_TRIS, STEP_N_PX)).reshape(-1, 1), u(0, 0.5, STEP_N_PX, 2), np.full((STEP_N_PX, 1), MARK, F)], 1))
    return dict(queue=q, state=state, virt=np.full((STEP_N_PX, 4), MARK, F), live=live, kind=name_of, word=word, tri=tri, **g)


def step_truth(sc, case, unfold, ops=None, lengths=None):
    """What k_chain_step<unfold> leaves: dict(albedo, normal, position, hits, state, virt: the arrays going in with what the truth says is written; rays:
    per slot the (o, d) the ray's survivor appends, `go` which slots have one; escaped, truncated: counts; r: specular_truth.step's dict of the consumed
    rays, `slots` their slot numbers)"""
    lengths = lengths or V.NumpyUnfold()
    q = case["queue"]
    slots = np.flatnonzero(case["live"] & (case["word"] >= 0) & (case["word"] < STEP_N_PX))
    L = case["word"][slots]
    assert len(np.unique(L)) == len(L)
    hit, o = q["hit"].reshape(-1, 4)[slots], q["o"].reshape(-1, 4)[slots]
    s0, s1 = case["state"][L, 0], case["state"][L, 1]
    r = S.step(sc, as_word(hit[:, 0]), hit[:, 1], hit[:, 2], s0[:, :3], s1[:, :3], as_word(s0[:, 3]), STEP_K, ray_origin=o[:, :3], length=s1[:, 3], ops=ops,
               unfold=lengths if unfold else None)
    out = {k: case[k].copy() for k in ("albedo", "normal", "position", "hits", "state", "virt")}
    end, go = ~r["go"], r["go"]
    e = L[end]
    for k in ("albedo", "normal", "position"):
        out[k][e, :3], out[k][e, 3] = r[k][end], 1
    out["hits"][e, 3] = r["cls"][end].astype(F)
    if unfold:
        on = end & ~r["escaped"]
        pv, valid = lengths.virtual_point(case["position"][L[on], :3], ORIGIN, r["length"][on])
        out["virt"][L[on], :3], out["virt"][L[on], 3] = pv, np.where(valid, r["length"][on], F(0))
    f = L[go]
    out["state"][f, 0, :3], out["state"][f, 0, 3] = r["T"][go], as_float(r["L"][go])
    out["state"][f, 1, :3], out["state"][f, 1, 3] = r["d"][go], r["length"][go] if unfold else F(0)
    n_slots = STEP_SEGMENTS * STEP_SEG_CAP
    ro, rd, has = np.zeros((n_slots, 4), F), np.zeros((n_slots, 4), F), np.zeros(n_slots, bool)
    has[slots[go]] = True
    ro[slots[go], :3], ro[slots[go], 3], rd[slots[go], :3], rd[slots[go], 3] = r["p"][go], TMIN, r["d"][go], as_float(f)
    return dict(out, rays=(ro, rd), go=has, escaped=int(r["escaped"].sum()), truncated=int(r["truncated"].sum()), r=r, slots=slots)


def step_reach(sc, case, t, unfold):
    """from the inputs and the truth: the queue holds what the case is named after, and the truth's verdicts cover every end a ray can take"""
    r, slots, counts = t["r"], t["slots"], case["queue"]["count"]
    live, word, kind = case["live"], case["word"], case["kind"][slots]
    ok = live.sum() == np.minimum(counts, STEP_SEG_CAP).sum() and (~live).any()
    if counts.sum() < 100:
        return bool(ok and counts.tolist() == [0, 1, 63] and len(slots) == 64)
    ok = ok and (counts > STEP_SEG_CAP).any() and all((word[live] == w).any() for w in BAD_L) and len(slots) == live.sum() - 6
    ok = ok and set(kind) == set(k[0] for k in RAY_KINDS)
    L_in = as_word(case["state"][word[slots], 0, 3])
    ok = ok and set(L_in[kind == "mirror"]) == set(range(STEP_K)) and r["escaped"][kind == "escaped"].all() and not r["escaped"][kind != "escaped"].any()
    mirror = kind == "mirror"
    ok = ok and r["go"][mirror & (L_in + 1 < STEP_K)].all() and r["truncated"][mirror & (L_in + 1 == STEP_K)].all() and (mirror & (L_in + 1 == STEP_K)).any()
    ok = ok and not r["go"][np.isin(kind, ("diffuse", "textured", "illum-0", "illum-2", "illum-8", "bad-material"))].any() and not r["truncated"][kind == "bad-material"].any()
    # glass: some rays refract, some are reflected whole (the truth's own dielectric says which)
    glass = np.flatnonzero(kind == "glass")
    hit = case["queue"]["hit"].reshape(-1, 4)[slots[glass]]
    n = S.hit_point(S.tri_words(sc, as_word(hit[:, 0])), hit[:, 1].copy(), hit[:, 2].copy())[1]
    refracted = S.dielectric(case["state"][word[slots[glass]], 1, :3], n, np.full(len(glass), F(1.5)))[1]
    ok = ok and refracted.any() and (~refracted).any() and (kind == "ior-0").sum() >= 2 and (r["normal"][kind == "zero-normal"] == 0).all()
    ok = ok and r["go"][(kind == "zero-normal") & (L_in + 1 < STEP_K) & (case["tri"][slots] == T_ZERO_N_MIRROR)].all()
    ok = ok and np.isnan(r["position"][kind == "nan-u"]).all() and (r["normal"][kind == "nan-u"] == 0).all()
    tex = r["albedo"][kind == "textured"]
    ok = ok and len(np.unique(tex.view(U32), axis=0)) > len(TEX_U)  # the texture's colours, not the material's one
    if unfold:
        on = ~r["go"] & ~r["escaped"]
        w = t["virt"][word[slots], 3]
        with np.errstate(invalid="ignore"):
            valid = (r["length"] > 0) & (r["length"] <= S.FINITE_MAX)
        ok = ok and np.isinf(r["length"][on]).any() and np.isnan(r["length"][on]).any() and (np.isfinite(r["length"]) & on & ~valid).any() and (w[on & ~valid] == 0).all()
        ok = ok and (w[on & valid] > 0).all()
        # the virtual point is the PRIMARY position's: built from the position the same thread then writes, it would be another point
        late = V.NumpyUnfold().virtual_point(r["position"][on], ORIGIN, r["length"][on])[0]
        fin = np.isfinite(r["length"][on]) & np.isfinite(late).all(-1)
        ok = ok and fin.sum() > 20 and (late[fin] != t["virt"][word[slots], :3][on][fin]).any(-1).all() and (t["virt"][word[slots], 3][r["escaped"]] == MARK).all()
    return bool(ok)


def wave_order_ok(slot_pixels, wave_of):
    """One wave's rays sit in consecutive slots in lane order: slot_pixels the pixel words of a segment's slots [0, count) in slot order, wave_of a function
    from a pixel word to (the wave that appended it, its lane)."""
    where = {}
    for slot, L in enumerate(slot_pixels):
        wave, lane = wave_of(int(L))
        where.setdefault(wave, []).append((slot, lane))
    for members in where.values():
        s = [m[0] for m in members]
        if s != list(range(s[0], s[0] + len(s))) or [m[1] for m in members] != sorted(m[1] for m in members):
            return False
    return True
