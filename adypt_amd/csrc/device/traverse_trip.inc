// One trip of the persistent CWBVH8 traversal loop — sections A-E of traversal.glsl:47-254 for the 64 rays of a wave.
// Textually included by k_trace (traverse.hpp) and k_path (path.hpp) inside their persistent loops: both kernels declare the per-lane ray
// state this code works on under the same names (od_x/od_y/od_z, idir, nx/ny/nz, octinv, tmin, hit_*, sp, ng_*, tg_*, node, pending, flush,
// active, ray, ...), `a` (lds_depth, stack_size, ray_stats), trip_nodes / trip_woop (the two base pointers), my_stack / my_spill / total_lanes, and the
// STATS / ANY constants, and two names for rays that end at their FIRST accepted triangle although the kernel's other rays do not (k_path's sun-visibility
// queries, traversal.glsl:257-494 semantics per lane): kTripShadowRays (constant: the kernel may carry such rays) and ADYPT_TRIP_SHADOW (this lane's ray is one).
// An include rather than a function: the traversal kernel sits exactly on its 80-register budget, and the register allocation of the two
// loops must not depend on what an inliner makes of a shared body.
		// No `if(active)` around the trip: a lane without a ray carries an inert state (no triangles, nothing pending, empty group,
		// empty stack), so every step below is a no-op for it — and it stays available as a TESTER of other lanes' triangles
		// (B / C), whose crossbar pulls need every lane of the wave enabled.
		{
			// One trip = at most one Woop test and at most one slab test per lane (a lane's triangles — up to three per trip — are tested
			// by whichever lanes of the wave are free: section B).  A lane whose node produced more triangles than the trip consumes keeps its already chosen next node pending
			// (fetched in the trip that slab-tests it): measured with adypt_get_wave_profile, an inner loop over all pairs ran
			// 2.4 iterations per trip with 6 of 64 lanes live — 40 % of the kernel's VALU slots at 9 % utilisation.
			// ---------------- A. choose the next node (traversal.glsl:47-66 / 245-250) unless one is pending ----------------
			// (flat sequence of predicated steps rather than nested branches: every nesting level made the compiler copy
			// the loop-carried ray state)
			const bool lane_any = ANY || (kTripShadowRays && (ADYPT_TRIP_SHADOW)); // this lane's ray ends at its first accepted triangle
			const bool can_pop = !pending && ng_y <= 0x00ffffffu && sp != 0;
			if(can_pop)
			{
				--sp;
				// two separate loads, each completed inside its branch: written as one select the compiler emits a single
				// flat_load (LDS or global decided by address) that waits on both memory counters; the LDS pop is the hot one.
				// Completing the pop here also means no older memory operation is pending when the triangle / node loads
				// below are issued.
				if(sp < a.lds_depth)
				{
					const uint2 g = my_stack[sp * 64];
					ng_x = g.x; ng_y = g.y;
					asm volatile("" : "+v"(ng_x), "+v"(ng_y));
				}
				else
				{
					const uint2 g = my_spill[(size_t)(sp - a.lds_depth) * total_lanes];
					ng_x = g.x; ng_y = g.y;
					asm volatile("" : "+v"(ng_x), "+v"(ng_y));
				}
			}
			const bool choose = !pending && ng_y > 0x00ffffffu;
			if(choose)
			{
				const uint32_t imask = ng_y;
				const uint32_t bit = 31u - (uint32_t)__builtin_clz(ng_y);
				ng_y &= ~(1u << bit);
				const uint32_t slot = (bit - 24u) ^ octinv;
				node = ng_x + (uint32_t)__builtin_popcount(imask & ~(0xffffffffu << slot));
				pending = true;
			}
			const bool push = choose && ng_y > 0x00ffffffu;
			const bool push_ok = push && sp < a.stack_size;
			if(push_ok)
			{
				if(sp < a.lds_depth) my_stack[sp * 64] = make_uint2(ng_x, ng_y);
				else my_spill[(size_t)(sp - a.lds_depth) * total_lanes] = make_uint2(ng_x, ng_y);
				++sp;
				if(STATS) depth_after_push = (uint32_t)sp;
			}
			if(ANY || kTripShadowRays) push_overflow |= push && !push_ok; // an any-hit ray may end before the visit the push belongs to
			else if(kOverflowPerRay) overflow |= push && !push_ok; // closest hit: the visit always follows, commit right away
			else any_overflow |= push && !push_ok;     // (k_path: nothing is reported per ray, the launch's flag takes it directly)
			// ---------------- B. hand the wave's triangles out, then issue every load of this trip back to back ----------------
			// The triangles the lanes have at hand — up to three per lane — form ONE list for the wave, a lane's triangles next to each other, and lane j
			// of the wave tests triangle j of the list, whoever owns it: the owner's ray comes through the LDS crossbar (ds_bpermute_b32: no memory —
			// but an issue slot of the SIMD like any vector instruction, profiles/r6_ablations.txt 3), the verdicts go back the same way and the owner applies them in the list's order — the sequential order of
			// traversal.glsl:213-243, so ties and any-hit termination stay bit-exact (a triangle's geometric test does not depend on the hit distance;
			// only its acceptance does, and that is decided by the owner).  Round 5's pair scheme (the second triangle to lane ^ 1 by DPP swaps) served
			// 72 % of the second triangles and no third one: 10 % of all lane-trips were lanes waiting for the rest of a node's triangles.
			// Place in the list: lanes below me count with every triangle they offer — three chained v_mbcnt pairs over the three ballots; which lane
			// owns entry j is found through a 64-byte table per wave (the owners write, the testers read: LDS executes a wave's operations in order).
			auto pull = [](uint32_t lane4, uint32_t v) { return (uint32_t)__builtin_amdgcn_ds_bpermute((int)lane4, (int)v); };
			auto pullf = [&](uint32_t lane4, float v) { return __uint_as_float(pull(lane4, __float_as_uint(v))); };
			// (x - 1 behind an empty-handed asm: as plain C the compiler takes `x != 0` from the subtraction's carry, turns that lane mask into a 0 / 1 register
			// and compares again for the ballot — two more vector instructions per mask)
			auto dec = [](uint32_t x) { uint32_t r; asm("v_add_u32_e32 %0, -1, %1" : "=v"(r) : "v"(x)); return r; };
			const uint32_t tg1 = tg_y & dec(tg_y), tg2 = tg1 & dec(tg1), tg3 = tg2 & dec(tg2); // the lane's triangles without the first one, two, three
			const bool has_tri = tg_y != 0;
			const unsigned long long m1 = __ballot(has_tri);
			unsigned long long m2 = __ballot(tg1 != 0), m3 = __ballot(tg2 != 0);
			const uint32_t cnt1 = (uint32_t)__popcll(m1);
			// (a list of more than 64: third triangles wait, then second ones — wave-uniform, scalar arithmetic)
			if(cnt1 + (uint32_t)__popcll(m2) + (uint32_t)__popcll(m3) > 64u) { m3 = 0ull; if(cnt1 + (uint32_t)__popcll(m2) > 64u) m2 = 0ull; }
			const uint32_t n_tests = cnt1 + (uint32_t)__popcll(m2) + (uint32_t)__popcll(m3);
			const bool own2 = tg1 != 0 && m2 != 0ull, own3 = tg2 != 0 && m3 != 0ull; // my second / third triangle is on the list
			const uint32_t base = __builtin_amdgcn_mbcnt_hi((uint32_t)(m3 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m3,
			                      __builtin_amdgcn_mbcnt_hi((uint32_t)(m2 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m2,
			                      __builtin_amdgcn_mbcnt_hi((uint32_t)(m1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m1, 0u))))));
			if(has_tri) trip_tab[base] = (uint8_t)lane;
			if(own2) trip_tab[base + 1u] = (uint8_t)(lane | 64);
			if(own3) trip_tab[base + 2u] = (uint8_t)(lane | 128);
			asm volatile("" ::: "memory");
			const bool do_test = (uint32_t)lane < n_tests;
			uint32_t ent;                                    // owner lane | ordinal << 6 of the triangle this lane tests
			asm volatile("" : "=v"(ent));                  // (only read under do_test; what a lane without a test pulls is never used)
			if(do_test) ent = trip_tab[lane];
			const uint32_t src4 = ent << 2;                  // (the crossbar takes bits 7..2 of the address)
			const uint32_t p_tgx = pull(src4, tg_x);
			uint32_t p_tgy = pull(src4, tg_y);
			const V2 t_od_x = v2(pullf(src4, od_x.x), pullf(src4, od_x.y)), t_od_y = v2(pullf(src4, od_y.x), pullf(src4, od_y.y)), t_od_z = v2(pullf(src4, od_z.x), pullf(src4, od_z.y));
			const float t_tmin = kUniformTmin ? tmin : pullf(src4, tmin); // (k_path, camera rays: every ray of the pass has the pass's tmin)
			if(ent >= 64u) p_tgy &= dec(p_tgy);
			if(ent >= 128u) p_tgy &= dec(p_tgy);
			const uint32_t tri_sel = p_tgx + (uint32_t)__builtin_ctz(p_tgy | 0x80000000u);
			tg_y = own3 ? tg3 : (own2 ? tg2 : tg1);          // consumed: what went onto the list
			float4 wp0, wp1, wp2;
			// registers only read under do_test / pending: "defined" by an empty asm (ADYPT_DEF4, canon_math.hpp: no instruction) instead of zero-filled —
			// leaving them uninitialised makes the register allocator spill, zero-filling costs VALU slots every trip
			ADYPT_DEF4(wp0); ADYPT_DEF4(wp1); ADYPT_DEF4(wp2);
			if(do_test)
			{
				const auto w0 = trip_woop + (size_t)tri_sel * 3;
				wp0 = trip_ld(w0); wp1 = trip_ld(w0 + 1); wp2 = trip_ld(w0 + 2);
			}
			uint4 n0, n1, n2, n3, n4;
			ADYPT_DEF4(n0); ADYPT_DEF4(n1); ADYPT_DEF4(n2); ADYPT_DEF4(n3); ADYPT_DEF4(n4);
			// The pending node is fetched in the trip that will slab-test it, i.e. once this trip's pair leaves no triangle behind.
			// A lane that still has triangles after the pair used to fetch its node again every trip (an L1 hit, but the vector
			// memory pipeline is as loaded as the vector ALU here — tools/microbench/l1_patterns.hip: a 16-byte-per-lane load costs
			// 16 cycles per CU at best and ~0.6 cycle per distinct cache line beyond that).
			if(pending && tg_y == 0)
			{
				const auto np = trip_nodes + (size_t)node * kNodeUint4;
				n0 = trip_ld(np); n1 = trip_ld(np + 1); n2 = trip_ld(np + 2); n3 = trip_ld(np + 3); n4 = trip_ld(np + 4);
			}
			__builtin_amdgcn_sched_barrier(0); // keep the compiler from hoisting arithmetic between the load issues

			// ---------------- C. triangles of the nodes visited last (traversal.glsl:213-243): one Woop test per lane ----------------
			float tt, tu, tv;
			asm volatile("" : "=v"(tt), "=v"(tu), "=v"(tv));
			bool geom_ok = false;
			if(do_test)
			{
				if(STATS) wave_event(2);
				// Woop test (traversal.glsl:219-242); (o·m, d·m) per row: x = dot3(origin, m.xyz), y = dot3(dir, m.xyz)
				// (the .y factor sits in the high half of the loaded (x, y) pair: pk_fma_hi reads it there)
				const V2 r0 = pk_fma(t_od_z, v2s(wp0.z), pk_fma_hi(t_od_y, v2(wp0.x, wp0.y), t_od_x * v2s(wp0.x)));
				const V2 r1 = pk_fma(t_od_z, v2s(wp1.z), pk_fma_hi(t_od_y, v2(wp1.x, wp1.y), t_od_x * v2s(wp1.x)));
				const V2 r2 = pk_fma(t_od_z, v2s(wp2.z), pk_fma_hi(t_od_y, v2(wp2.x, wp2.y), t_od_x * v2s(wp2.x)));
				const float toz = wp0.w - r0.x;
				const float tidz = rcp_ieee(r0.y);
				tt = toz * tidz;
				tu = fmaf(tt, r1.y, wp1.w + r1.x);
				tv = fmaf(tt, r2.y, wp2.w + r2.x);
				geom_ok = tt > t_tmin && tu >= 0.0f && tu <= 1.0f && tv >= 0.0f && tu + tv <= 1.0f;
			}
			// The verdicts on my triangles sit in lanes base, base + 1, base + 2 (NaN = rejected).  Applied in the list's order with the shortened hit_t;
			// any-hit: nothing counts after the first accepted triangle (traversal.glsl:477-483).  The winner's (u, v, reference index) follow by a second pull.
			const float verdict = geom_ok ? tt : __builtin_nanf("");
			const uint32_t b4 = base << 2;
			const float v0 = pullf(b4, verdict), v1 = pullf(b4 + 4u, verdict), v2_ = pullf(b4 + 8u, verdict);
			uint32_t win4 = b4 + 12u; // (a lane that is none of my testers: "nothing accepted")
			bool won = false;
			uint32_t n_seen = has_tri ? 1u : 0u; // STATS: triangles the sequential loop would have tested
			if(ANY || STATS || kTripShadowRays)
			{
				if(has_tri && v0 < hit_t) { hit_t = v0; win4 = b4; won = true; }
				if(own2 && !(lane_any && won)) { n_seen = 2u; if(v1 < hit_t) { hit_t = v1; win4 = b4 + 4u; won = true; } }
				if(own3 && !(lane_any && won)) { n_seen = 3u; if(v2_ < hit_t) { hit_t = v2_; win4 = b4 + 8u; won = true; } }
			}
			else
			{
				// the same three steps under EXEC: the lanes that offer a k-th triangle, narrowed by the compare itself (v_cmpx writes EXEC), take the
				// verdict and its tester's address with two full-rate moves — 9.3 issue cycles per step where compare + mask + two selects take 15.4
				unsigned long long ex;
				asm volatile("s_mov_b64 %[ex], exec\n\t"
				             "s_and_b64 exec, %[ex], %[m1]\n\tv_cmpx_lt_f32_e32 vcc, %[v0], %[t]\n\tv_mov_b32_e32 %[t], %[v0]\n\tv_mov_b32_e32 %[w], %[b4]\n\t"
				             "s_and_b64 exec, %[ex], %[m2]\n\tv_cmpx_lt_f32_e32 vcc, %[v1], %[t]\n\tv_mov_b32_e32 %[t], %[v1]\n\tv_add_u32_e32 %[w], 4, %[b4]\n\t"
				             "s_and_b64 exec, %[ex], %[m3]\n\tv_cmpx_lt_f32_e32 vcc, %[v2], %[t]\n\tv_mov_b32_e32 %[t], %[v2]\n\tv_add_u32_e32 %[w], 8, %[b4]\n\t"
				             "s_mov_b64 exec, %[ex]"
				             : [t] "+v"(hit_t), [w] "+v"(win4), [ex] "=&s"(ex)
				             : [v0] "v"(v0), [v1] "v"(v1), [v2] "v"(v2_), [b4] "v"(b4), [m1] "s"(m1), [m2] "s"(m2), [m3] "s"(m3)
				             : "vcc", "scc");
				won = win4 != b4 + 12u;
			}
			{
				const float w_u = pullf(win4, tu), w_v = pullf(win4, tv);
				const uint32_t w_idx = pull(win4, tri_sel);
				if(won) { ADYPT_TRIP_TAKE_HIT(w_u, w_v, w_idx); }
			}
			if(STATS) n_tris += n_seen;
			if((ANY || kTripShadowRays) && lane_any && won) { tg_y = 0; pending = false; }

			if(tg_y != 0)
			{
				// more triangles of this node: next trip (the pending node is fetched in the trip that consumes the last of them)
			}
			else if(pending)
			{
				// ---------------- D. slab tests of the fetched node (traversal.glsl:69-205) ----------------
				pending = false;
				if(ANY || kTripShadowRays) overflow |= push_overflow;
				if(STATS) wave_event(4);
				if(STATS) { ++n_nodes; hash = (hash * 0x01000193u) ^ node; max_depth = max(max_depth, depth_after_push); }
				// octinv replicated into the 4 bytes: v_perm_b32 with selector 0 instead of a quarter-rate v_mul_lo_u32
				const uint32_t octinv4 = __builtin_amdgcn_perm(0u, octinv, 0u);
				const uint32_t head_w = n0.w;
				const float aix = exp_byte<0>(head_w) * idir.x; // uintBitsToFloat(e << 23) * idir (traversal.glsl:76-79)
				const float aiy = exp_byte<1>(head_w) * idir.y;
				const float aiz = exp_byte<2>(head_w) * idir.z;
				const float aox = (__uint_as_float(n0.x) - od_x.x) * idir.x;
				const float aoy = (__uint_as_float(n0.y) - od_y.x) * idir.y;
				const float aoz = (__uint_as_float(n0.z) - od_z.x) * idir.z;
				ng_x = n1.x;
				tg_x = n1.y;
				uint32_t hitmask = 0;
#pragma unroll
				for(int g = 0; g < 2; ++g)
				{
					const uint32_t meta4 = g ? n1.w : n1.z;
					const uint32_t is_inner4 = (meta4 & (meta4 << 1)) & 0x10101010u;
					// per-byte select mask for octinv (<= 7): (b << 3) - b = 7 for inner bytes, no cross-byte borrow (the compiler emits one
					// v_mul_lo_u32 by 7: measured 1.4x the issue cost of an add on gfx950 — cheaper than two shift-ors)
					const uint32_t inner1 = is_inner4 >> 4;
					// (bits 5-7 of a byte stay: the only use of a byte of this word is as the shift count of shl_bytes, which takes its low 5 bits)
					const uint32_t bit_index4 = meta4 ^ (octinv4 & ((inner1 << 3) - inner1));
					const uint32_t child_bits4 = (meta4 >> 5) & 0x07070707u;
					const uint32_t qlox = g ? n2.y : n2.x, qloy = g ? n2.w : n2.z, qloz = g ? n3.y : n3.x;
					const uint32_t qhix = g ? n3.w : n3.z, qhiy = g ? n4.y : n4.x, qhiz = g ? n4.w : n4.z;
					const uint32_t slox = nx ? qhix : qlox, shix = nx ? qlox : qhix;
					const uint32_t sloy = ny ? qhiy : qloy, shiy = ny ? qloy : qhiy;
					const uint32_t sloz = nz ? qhiz : qloz, shiz = nz ? qloz : qhiz;
					// what child j raises in the hit mask: child_bits << bit_index, byte j of both words in one SDWA shift
					const uint32_t raise[4] = {shl_bytes<0>(bit_index4, child_bits4), shl_bytes<1>(bit_index4, child_bits4), shl_bytes<2>(bit_index4, child_bits4), shl_bytes<3>(bit_index4, child_bits4)};
#pragma unroll
					for(int j = 0; j < 4; ++j)
					{
						const int sh = 8 * j;
						// (entry, exit) distance of one axis in one v_pk_fma_f32: t = fma(float(q), adj_idir, adj_org)
						const V2 tx = pk_fma(v2((float)((slox >> sh) & 0xffu), (float)((shix >> sh) & 0xffu)), v2s(aix), v2s(aox));
						const V2 ty = pk_fma(v2((float)((sloy >> sh) & 0xffu), (float)((shiy >> sh) & 0xffu)), v2s(aiy), v2s(aoy));
						const V2 tz = pk_fma(v2((float)((sloz >> sh) & 0xffu), (float)((shiz >> sh) & 0xffu)), v2s(aiz), v2s(aoz));
						const float cmin = fmaxf(fmaxf(tx.x, ty.x), max_num(tz.x, tmin));   // IEEE maxNum / minNum
						const float cmax = fminf(fminf(tx.y, ty.y), min_num(tz.y, hit_t));
						or_if_le(hitmask, cmin, cmax, raise[j]);
					}
				}
				ng_y = (hitmask & 0xff000000u) | (head_w >> 24);
				tg_y = hitmask & 0x00ffffffu;
			}
			// ---------------- E. ray finished (traversal.glsl:245-254)? ----------------
			// Nothing left to test, to visit or to pop — checked in the SAME trip as the slab test that found no child
			// (or the triangle tests that were the last work): a separate trip just to notice it cost one of ~13 trips per ray.
			if(active && tg_y == 0 && !pending && ((ng_y <= 0x00ffffffu && sp == 0) || ((ANY || kTripShadowRays) && lane_any && won)))
			{
				if(ANY || kTripShadowRays) { if(lane_any) { ng_y = 0; sp = 0; } } // an any-hit ray ends with work left: make the lane inert
				flush = true; // the hit (k_trace: registers; k_path: the path's table slot) and `ray` stay where they are until the refill / exchange (or the exit) takes them
				any_overflow |= overflow;
				if(STATS)
				{
					if(a.ray_stats)
					{
						RayStats rs;
						rs.ref_idx = hit_idx; rs.nodes = n_nodes; rs.tris = n_tris; rs.hash = hash;
						rs.max_depth = overflow ? 0xffffffffu : max_depth; rs.pad0 = rs.pad1 = rs.pad2 = 0;
						a.ray_stats[ray] = rs;
					}
					st_nodes += n_nodes; st_tris += n_tris; st_hits += hit_idx != -1 ? 1 : 0;
					st_maxdepth = max(st_maxdepth, max_depth);
				}
				active = false;
			}
		}
