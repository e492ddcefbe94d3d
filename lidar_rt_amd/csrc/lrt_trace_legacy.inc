// lrt_trace_legacy.inc -- the K-buffer packet kernel k_trace<BWD> (fwd_mode = 0 / bwd_mode = 0, and the re-tracing
// backward that every other mode falls back to when the hit record overflowed); included by lrt_kernels.hip.

#define CSWAP(a, b) do { unsigned lo_ = (a) < (b) ? (a) : (b); unsigned hi_ = (a) < (b) ? (b) : (a); (a) = lo_; (b) = hi_; } while (0)

template <bool BWD>
__global__ void __launch_bounds__(256, 2) k_trace(const TraceParams p, const float* __restrict__ g_rec,
                                                const float* __restrict__ g_nodes)
{
    __shared__ float s_t[4][LRT_CHUNK][64];
    __shared__ int   s_g[4][LRT_CHUNK][64];
    __shared__ float s_a[4][LRT_CHUNK][64];
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int TWm = (1 << p.tw_log2) - 1;
    const int TH = 64 >> p.tw_log2;
    const float bg0 = p.bg[0], bg1 = p.bg[1], bg2 = p.bg[2];
    const int nsh = p.nsh;
    unsigned st_cand = 0, st_comp = 0, st_pass = 0, st_nodes = 0, st_prims = 0, st_ins = 0;
    unsigned long long st_clk_sum = 0, st_clk_max = 0;
    if (BWD && p.guard != 0) {               // stream-ordered backward: the re-trace runs only if the hit record cannot be used
        const bool bad = (*p.hit_ovf != 0) || (*p.n_hits_dev > p.n_spec);
        if ((p.guard == 1) == bad) return;
    }

    // Persistent wavefronts with XCD-aware work distribution: the tile grid is cut into 8 contiguous azimuth
    // sectors, one queue per XCD (workgroup b is observed to run on XCD b % 8 -- used for L2 locality only, any
    // placement is correct).  A wave drains its own XCD's queue first, then steals from the others.
    unsigned q = blockIdx.x & 7u; int q_tried = 0;
    for (;;) {
        const int c0 = (int)(q * (unsigned)p.tiles_x) >> 3, c1 = (int)((q + 1u) * (unsigned)p.tiles_x) >> 3;
        const unsigned nq = (unsigned)((c1 - c0) * p.tiles_y);
        unsigned ti = 0;
        if (lane == 0) ti = atomicAdd(p.tile_counter + q, 1u);
        ti = __builtin_amdgcn_readfirstlane(ti);
        if (ti >= nq) {
            if (++q_tried == 8) break;
            q = (q + 1u) & 7u;
            continue;
        }
        const int ty = (int)(ti % (unsigned)p.tiles_y), tx = c0 + (int)(ti / (unsigned)p.tiles_y);
        const unsigned long long clk0 = p.stats ? wall_clock64() : 0ull;
        const int h = ty * TH + (lane >> p.tw_log2), w = (tx << p.tw_log2) + (lane & TWm);
        const bool valid = (h < p.H) && (w < p.W);
        const size_t r = valid ? ((size_t)h * p.W + w) : 0;
        float o[3], d[3], inv[3];
        for (int i = 0; i < 3; i++) { o[i] = p.ray_o[3 * r + i]; d[i] = p.ray_d[3 * r + i]; inv[i] = 1.0f / d[i]; }
        float b[16];
        lrt_sh_basis(p.deg, d, b);

        float T = 1.f, C0 = 0.f, C1 = 0.f, C2 = 0.f, Dd = 0.f, Wt = 0.f, N0 = 0.f, N1 = 0.f, N2 = 0.f;
        float go[3] = {0.f, 0.f, 0.f}, gd[3] = {0.f, 0.f, 0.f};      // BWD: the ray's gradient (p.d_ray_o)
        float dL[LRT_NCH], fin[LRT_NCH], dL_dbg = 0.f;
        if (BWD) {
            for (int i = 0; i < LRT_NCH; i++) { dL[i] = p.dL_dout[LRT_NCH * r + i]; fin[i] = p.out9_in[LRT_NCH * r + i]; }
            dL_dbg = dL[0] * bg0 + dL[1] * bg1 + dL[2] * bg2;
        }
        float base = __uint_as_float(__float_as_uint(LRT_T_NEAR) - 1u);   // accept t >= 0.2 (forward.cu:214)
        bool done = !valid;
        int dbg_n = 0, n_rec = 0;

        bool is_near = false;                       // a quad closer than 0.2 m -> the ray is resolved by the near-ray replay (k_fwd_near; the last workgroup of the backward)
        for (int pass = 0; pass < 4096; ++pass) {   // hard bound (65k hits per ray) so a bug can never hang the GPU
            const bool act = !done;
            if (!__any(act)) break;
            st_pass++;
            // ---- per-lane 16-slot nearest-hit buffer (params.h:83-97), ascending in t
            float kt[LRT_CHUNK], ka[LRT_CHUNK]; int kg[LRT_CHUNK];
#pragma unroll
            for (int i = 0; i < LRT_CHUNK; i++) { kt[i] = 1e16f; kg[i] = 0; ka[i] = 0.f; }
            unsigned cnt = 0;

            // ---- packet traversal; stack entry = (is_leaf << 31) | index, kept in lane sp of one VGPR
            int stk = 0; int sp = 0;
            sp = 1;                                                         // root = node 0 in lane 0 (stk == 0)
            while (sp > 0) {
                sp--;
                const unsigned e = (unsigned)__builtin_amdgcn_readlane(stk, sp);
                if (e & 0x80000000u) {
                    // ---------------- leaf: every ray of the tile tests every quad of the leaf.
                    // ONE coalesced 512-B vector load fetches the 8 records (lane L holds float4 #L%4 of quad L/4);
                    // each record is then broadcast to SGPRs with v_readlane (one memory round trip per leaf, not per quad).
                    const int k0 = (int)(e & 0x7fffffffu) * LRT_LEAF;
                    float4 lv = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (lane < 4 * LRT_LEAF) lv = reinterpret_cast<const float4*>(g_rec)[(size_t)k0 * 4 + lane];
                    for (int j = 0; j < LRT_LEAF; ++j) {
                        const int l0 = 4 * j;
                        // staged test, cheapest rejection first; every stage ends in a wave-uniform early-out
                        const float flim = rdl(lv.w, l0 + 1);
                        if (!(flim > 0.f)) continue;                                    // unhittable / padding record
                        st_prims++;
                        const float nx = rdl(lv.x, l0), ny = rdl(lv.y, l0), nz = rdl(lv.z, l0);
                        const float cx = rdl(lv.x, l0 + 1) - o[0], cy = rdl(lv.y, l0 + 1) - o[1], cz = rdl(lv.z, l0 + 1) - o[2];
                        const float t = (nx * cx + ny * cy + nz * cz) / (nx * d[0] + ny * d[1] + nz * d[2]);
                        bool hit = act && (t > base) && (t < kt[LRT_CHUNK - 1]);         // anyhit: forward.cu:323 (base: 0.2 m in the first pass)
                        const bool nearc = (!BWD || p.near_list != nullptr) && act && pass == 0 && (t > 0.f) && (t < LRT_T_NEAR);   // candidate for the stale-slot rule
                        if (!__any(hit || nearc)) continue;
                        const float px = t * d[0] - cx, py = t * d[1] - cy, pz = t * d[2] - cz;   // x - mu
                        if (__any(nearc)) {
                            const float un = rdl(lv.x, l0 + 2) * px + rdl(lv.y, l0 + 2) * py + rdl(lv.z, l0 + 2) * pz;
                            const float vn = rdl(lv.x, l0 + 3) * px + rdl(lv.y, l0 + 3) * py + rdl(lv.z, l0 + 3) * pz;
                            is_near = is_near || (nearc && (fabsf(un) <= flim) && (fabsf(vn) <= flim));
                            if (!__any(hit)) continue;
                        }
                        const float u = rdl(lv.x, l0 + 2) * px + rdl(lv.y, l0 + 2) * py + rdl(lv.z, l0 + 2) * pz;
                        hit = hit && (fabsf(u) <= flim);
                        if (!__any(hit)) continue;
                        const float v = rdl(lv.x, l0 + 3) * px + rdl(lv.y, l0 + 3) * py + rdl(lv.z, l0 + 3) * pz;
                        hit = hit && (fabsf(v) <= flim);
                        if (__any(hit)) {
                            st_ins++;
                            if (hit) {
                                cnt++;
                                float ct = t, ca = rdl(lv.w, l0) * expf(-0.5f * (u * u + v * v));   // op * G, un-clamped
                                int cg = __float_as_int(rdl(lv.w, l0 + 2));
#pragma unroll
                                for (int i = 0; i < LRT_CHUNK; i++) {                 // sorted insert, forward.cu:336-352
                                    const bool sw = kt[i] > ct;
                                    const float tt = kt[i], ta = ka[i]; const int tg = kg[i];
                                    kt[i] = sw ? ct : tt; ka[i] = sw ? ca : ta; kg[i] = sw ? cg : tg;
                                    ct = sw ? tt : ct; ca = sw ? ta : ca; cg = sw ? tg : cg;
                                }
                            }
                        }
                    }
                } else {
                    // ---------------- inner node: 8 child boxes (SoA), slab test per lane, ballot per child
                    typedef float f16v __attribute__((ext_vector_type(16)));
                    const f16v* ndv = static_cast<const f16v*>(__builtin_assume_aligned(g_nodes + (size_t)e * LRT_NODE_FLOATS, 256));
                    const f16v nA = ndv[0], nB = ndv[1], nC = ndv[2];               // 3 x s_load_dwordx16: lo.x lo.y | lo.z hi.x | hi.y hi.z
                    const float2 nH = *reinterpret_cast<const float2*>(g_nodes + (size_t)e * LRT_NODE_FLOATS + 48);
                    float nd[48];
#pragma unroll
                    for (int i = 0; i < 16; i++) { nd[i] = nA[i]; nd[16 + i] = nB[i]; nd[32 + i] = nC[i]; }
                    const unsigned cbase = (unsigned)__float_as_int(nH.x);
                    const unsigned cleaf = (unsigned)__float_as_int(nH.y) << 31;
                    const float tfar = kt[LRT_CHUNK - 1];
                    unsigned key[8]; int nh = 0;
                    st_nodes++;
#pragma unroll
                    for (int c = 0; c < 8; c++) {
                        const float t0x = (nd[c] - o[0]) * inv[0], t1x = (nd[24 + c] - o[0]) * inv[0];
                        const float t0y = (nd[8 + c] - o[1]) * inv[1], t1y = (nd[32 + c] - o[1]) * inv[1];
                        const float t0z = (nd[16 + c] - o[2]) * inv[2], t1z = (nd[40 + c] - o[2]) * inv[2];
                        const float tn = fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fminf(t0z, t1z));
                        const float tf = fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fmaxf(t0z, t1z));
                        // the forward's first pass also walks the boxes in front of 0.2 m: a quad there makes the ray a near ray (k_fwd_near)
                        const float tb = (!BWD && pass == 0) ? 0.f : base;
                        const bool hit = (p.no_cull & 1) ? (nd[c] < LRT_EMPTY) : (act && (tf >= fmaxf(tn, tb)) && (tn <= tfar));
                        const unsigned long long m = __ballot(hit);
                        unsigned kk = 0xffffffffu;
                        if (m) {
                            const int first = __ffsll((long long)m) - 1;
                            const unsigned kb = (unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(fmaxf(tn, 0.f)), first);
                            kk = (p.no_cull & 2) ? (unsigned)c : ((kb & ~7u) | (unsigned)c);
                            nh++;
                        }
                        key[c] = kk;
                    }
                    // sort the (distance | child) keys ascending: 19-comparator network, all wave-uniform
                    CSWAP(key[0], key[1]); CSWAP(key[2], key[3]); CSWAP(key[4], key[5]); CSWAP(key[6], key[7]);
                    CSWAP(key[0], key[2]); CSWAP(key[1], key[3]); CSWAP(key[4], key[6]); CSWAP(key[5], key[7]);
                    CSWAP(key[1], key[2]); CSWAP(key[5], key[6]); CSWAP(key[0], key[4]); CSWAP(key[3], key[7]);
                    CSWAP(key[1], key[5]); CSWAP(key[2], key[6]);
                    CSWAP(key[1], key[4]); CSWAP(key[3], key[6]);
                    CSWAP(key[2], key[4]); CSWAP(key[3], key[5]);
                    CSWAP(key[3], key[4]);
#pragma unroll
                    for (int j = 7; j >= 0; j--) {                                    // farthest first -> nearest pops first
                        if (j < nh) {
                            const unsigned ent = cleaf | (cbase + (key[j] & 7u));
                            stk = (lane == sp) ? (int)ent : stk;                    // v_writelane equivalent (uniform ent, sp)
                            sp++;
                        }
                    }
                }
            }

            // ---- stage the sorted chunk through LDS so the consume loop can be a real loop
#pragma unroll
            for (int i = 0; i < LRT_CHUNK; i++) { s_t[wv][i][lane] = kt[i]; s_g[wv][i][lane] = kg[i]; s_a[wv][i][lane] = ka[i]; }
            const int nv = (int)min(cnt, (unsigned)LRT_CHUNK);
            bool stop = false; float last_t = base;
            for (int i = 0; i < LRT_CHUNK; ++i) {
                const bool on = act && !stop && (i < nv) && !is_near;       // a near ray is not composited here (k_fwd_near does it)
                if (!__any(on)) break;
                if (on) {
                    const float t = s_t[wv][i][lane]; const int g = s_g[wv][i][lane]; const float ao = s_a[wv][i][lane];
                    last_t = t;
                    if (p.dbg && dbg_n < 32) { p.dbg[r * 64 + 2 * dbg_n] = t; p.dbg[r * 64 + 2 * dbg_n + 1] = __int_as_float(g); dbg_n++; }
                    st_cand++;
                    const float alpha = fminf(LRT_ALPHA_MAX, ao);                       // forward.cu:247
                    if (alpha >= LRT_ALPHA_MIN) {
                        const float testT = T * (1.f - alpha);
                        if (testT < LRT_T_STOP) {
                            stop = true;                                                // forward.cu:253-257
                        } else {
                            const float wgt = alpha * T;
                            st_comp++;
                            if (!BWD) {
                                float c0, c1, c2; bool cl0;
                                sh_colour(p, g, b, nsh, c0, c1, c2, cl0);
                                C0 += wgt * c0; C1 += wgt * c1; C2 += wgt * c2;
                                Dd += wgt * t; Wt += wgt;
                                if (p.accum) unsafeAtomicAdd(p.accum + g, wgt);         // forward.cu:268 (null: option deferred_accum)
                                if (p.hit_t) {                                          // record for the replay backward
                                    if (n_rec < p.hit_cap) {
                                        const size_t id = r * (size_t)p.hit_cap + n_rec;
                                        p.hit_t[id] = t; p.hit_g[id] = g;
                                    }
                                    n_rec++;
                                }
                            } else {
                                RayAcc a = {T, C0, C1, C2, Dd, Wt, N0, N1, N2, {go[0], go[1], go[2]}, {gd[0], gd[1], gd[2]}};
                                bwd_hit<true, true>(p, o, d, b, nsh, dL, fin, dL_dbg, t, g, ao, a);
                                C0 = a.C0; C1 = a.C1; C2 = a.C2; Dd = a.Dd; N0 = a.N0; N1 = a.N1; N2 = a.N2;
                                for (int i2 = 0; i2 < 3; i2++) { go[i2] = a.go[i2]; gd[i2] = a.gd[i2]; }
                            }
                            T = testT;
                        }
                    }
                }
            }
            if (act) {
                if (stop || cnt < (unsigned)LRT_CHUNK || is_near) done = true;           // forward.cu:282-285
                else base = last_t + LRT_STEP_EPS;                                      // forward.cu:288
            }
        }

        if (p.stats) { const unsigned long long dc = wall_clock64() - clk0; st_clk_sum += dc; st_clk_max = dc > st_clk_max ? dc : st_clk_max; }
        if (!BWD && valid && is_near) { const unsigned ix = atomicAdd(p.near_count, 1u); p.near_list[ix] = (int)r; n_rec = 0; }
        if (BWD && valid && is_near && p.near_list) { const unsigned ix = atomicAdd(p.near_count, 1u); p.near_list[ix] = (int)r; }      // replayed below
        if (BWD && valid && !is_near && p.d_ray_o) store_ray_grad(p, r, go, gd);                                                  // (a near ray: by the replay)
        if (!BWD && valid && p.hit_t) {
            p.hit_n[r] = min(n_rec, p.hit_cap); if (n_rec > p.hit_cap) atomicOr(p.hit_ovf, 1);
            if (p.hit_count) atomicAdd(p.hit_count, (unsigned)min(n_rec, p.hit_cap));     // no return value: fire and forget
        }
        if (!BWD && valid) {
            float* op_ = p.out9 + LRT_NCH * r;
            op_[0] = C0 + T * bg0; op_[1] = C1 + T * bg1; op_[2] = C2 + T * bg2;
            op_[3] = Dd; op_[4] = Wt; op_[5] = 0.f; op_[6] = 0.f; op_[7] = 0.f; op_[8] = T;
        }
    }
    if (BWD && p.near_list) {
        // Rays with a quad closer than 0.2 m were left out above (the 16-slot buffer's stale-slot rule cannot be expressed per packet,
        // lrt_near.inc) and listed; the LAST workgroup to get here replays them, one wave, ray by ray (normally the list is empty).
        __shared__ NearLds s_near;
        __shared__ unsigned s_last;
        __threadfence();
        __syncthreads();
        if (threadIdx.x == 0) s_last = (atomicAdd(p.near_done, 1u) == gridDim.x - 1u) ? 1u : 0u;
        __syncthreads();
        if (s_last && wv == 0) {
            __threadfence();
            const unsigned n_near = min(__hip_atomic_load(p.near_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), (unsigned)p.H * (unsigned)p.W);
            for (unsigned qi = 0; qi < n_near; ++qi) near_replay<true>(p, g_rec, p.naos, __hip_atomic_load(p.near_list + qi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), 0, lane, s_near);
        }
    }
    if (p.stats) {
        if (lane == 0) { atomicAdd(p.stats + 5, st_clk_sum); atomicMax(p.stats + 6, st_clk_max); atomicAdd(p.stats + 7, (unsigned long long)st_ins); }
        const unsigned a = wave_sum_u(st_cand), c = wave_sum_u(st_comp);
        if (lane == 0) {
            atomicAdd(p.stats + 0, (unsigned long long)a); atomicAdd(p.stats + 1, (unsigned long long)c);
            atomicAdd(p.stats + 2, (unsigned long long)st_pass); atomicAdd(p.stats + 3, (unsigned long long)st_nodes);
            atomicAdd(p.stats + 4, (unsigned long long)st_prims);
        }
    }
}

