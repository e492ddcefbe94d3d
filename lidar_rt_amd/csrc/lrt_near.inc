// lrt_near.inc -- rays with a quad closer than 0.2 m to their origin: a literal replay of the reference's 16-slot K-buffer
// (included by lrt_kernels.hip after the trace kernels).
//
// The reference's raygen loop skips a hit with depth < 0.2 BEFORE it clears the hit's buffer slot (forward.cu:214 precedes
// :218-219).  The slot therefore survives the restart behind the 16th candidate with its OLD, small tmx: it sorts to the front of
// the next chunk, is evaluated at the fictitious depth tmx + payload.dpt (normally far from its Gaussian: alpha < 1/255, no
// contribution), takes a place among the 16 that a real hit would have had, and -- because `cnt` only counts the NEW any-hit
// insertions while the loop stops at i >= cnt -- the last real hits of the chunk are never looked at; with cnt < 16 the ray ends.
// None of this can be expressed in the collect-and-resolve formulation, so the trace kernels only LIST such rays (normal scenes
// have none; geometry stays away from the sensor) and this kernel replays them: one wave per ray collects the quads the ray hits
// (own traversal: depth slab by depth slab as the loop asks for candidates in the production forward, all at once for the literal
// one-lane consumers), sorts them by (t, gidx), and runs the reference's loop literally, with the any-hit program fed in ascending
// order of t.  (OptiX feeds it in BVH order, which decides `cnt` in the presence of stale slots: the reference
// itself is order-dependent there; ascending order is the choice the oracle's `sorted_anyhit` switch reproduces.)
#define NEAR_CAP 1024
#ifndef NEAR_NB
#define NEAR_NB 4                         // sub-batches of eight stack entries per step of the walk
#endif
#define NEAR_STACK 1024                   // entries; a step pops up to 8 and pushes up to 64

__device__ __forceinline__ float near_alpha(const float* __restrict__ rc, const float* o, const float* d, float dpt, bool& skip)
{
    // compute_transmat_uv at xyz = o + dpt d (forward.cu:209-246); rc = the quad's 64-byte record
    const float x0 = o[0] + dpt * d[0], x1 = o[1] + dpt * d[1], x2 = o[2] + dpt * d[2];
    const float p0 = x0 - rc[4], p1 = x1 - rc[5], p2 = x2 - rc[6];
    const float u = rc[8] * p0 + rc[9] * p1 + rc[10] * p2, v = rc[12] * p0 + rc[13] * p1 + rc[14] * p2;
    const float cosv = -((rc[4] - o[0]) * rc[0] + (rc[5] - o[1]) * rc[1] + (rc[6] - o[2]) * rc[2]);
    skip = (cosv == 0.f);
    return rc[3] * expf(-0.5f * (u * u + v * v));             // opacity x G, un-clamped
}

// LDS working set of one replaying wave (20 KB: eight waves per CU)
// (round 6: the Gaussian of a hit, which only breaks ties of equal depths, is read from the hit's record when a tie exists: 20 KB per wave, eight waves per CU
// instead of six)
struct NearLds { float t[NEAR_CAP], ts[NEAR_CAP]; int s[NEAR_CAP], ss[NEAR_CAP]; unsigned stack[NEAR_STACK]; };
// the sorted stream of a ray's hits and where its collection stands: the hits with t < b_hi are in ts / ss [0, n); more = geometry at or beyond b_hi exists
struct NearSt { int n; float b_hi; int more; int ovf; };
#ifndef NEAR_SLAB0
#define NEAR_SLAB0 1.5f                   // first depth slab of the production forward's lazy collection (then x 4 per refill, unbounded after five)
#endif

// The reference's raygen loop (forward.cu:195-292) with its 16-slot K-buffer held ACROSS 16 LANES (round 6; the deferred-colour forward).  The literal
// one-lane loop below spends its time in two chains: the any-hit insertion (16 compare-and-swap steps per candidate) and, per consumed slot, the
// dependent load of the slot's record followed by the exponential -- ~100 hits x 2 us of memory latency per near ray, 5.5 ms for the 50 k near rays of
// a sensor 0.1 m from a surface.  Here lane i holds slot i:
//   * insertion: the window is sorted whenever the any-hit program runs (the slots a restart leaves behind are the near-skipped ones, which are
//     the smallest and sit at the front, followed by cleared slots at 1e16), so a candidate's place is the number of slots not larger than it (one
//     ballot) and the slots behind it move up by one lane -- the same result as the reference's pass of conditional swaps;
//   * consumption: the 16 lanes fetch their slots' records and evaluate depth, alpha and the skip conditions AT ONCE (one memory round trip per
//     chunk instead of sixteen); the decisions that depend on each other (last_gidx, the transmittance stop) then walk the lanes' results with
//     v_readlane, no memory in between.
// Side effects (accum, hit record, overflow list) are issued by lane 0.  Every scalar of the loop is kept identical in all lanes.
// The quads the ray hits with t in [b_lo, st.b_hi), appended to the sorted stream (they all lie behind what the stream holds).  The walk: up to 8 NEAR_NB stack
// entries per step, lane (e, c) = child / quad c of entry e, as sub-batches of eight whose loads go out together -- a chain of dependent memory round trips, one
// per step (round 4 popped one entry per step and used 8 of the 64 lanes: ~300 dependent loads per ray, 210 us per ray: profiles/r05_near_rays.md).  The order
// of the visit is irrelevant: the new hits are rank-sorted by (t, gidx).  A child box is entered when the ray's interval in it overlaps the slab; `more` reports a
// box the ray is inside at or beyond b_hi.
__device__ __forceinline__ NearSt near_collect(const float* __restrict__ g_rec, const float* __restrict__ g_naos, NearLds& L, const float* o, const float* d, const float* inv,
                                               int lane, NearSt st, float b_lo)
{
    float* const s_t = L.t; float* const s_ts = L.ts; int* const s_s = L.s; int* const s_ss = L.ss; unsigned* const s_stack = L.stack;
    const unsigned long long below = (1ull << lane) - 1ull;
    const float b_hi = st.b_hi;
    int sp = 1, n = 0; bool ovf = false, beyond = false;
    if (lane == 0) s_stack[0] = 0u;
    const int grp = lane >> 3, c = lane & 7;
    while (sp > 0 && !ovf) {
        const int take = sp < 8 * NEAR_NB ? sp : 8 * NEAR_NB;
        sp -= take;
        unsigned e2[NEAR_NB]; bool has2[NEAR_NB];
#pragma unroll
        for (int b = 0; b < NEAR_NB; b++) { has2[b] = grp + 8 * b < take; e2[b] = has2[b] ? s_stack[sp + 8 * b + grp] : 0u; }
        float4 q0[NEAR_NB], q1[NEAR_NB], q2[NEAR_NB], q3[NEAR_NB];
#pragma unroll
        for (int b = 0; b < NEAR_NB; b++) {
            q0[b] = q1[b] = q2[b] = q3[b] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (has2[b] && (e2[b] & 0x80000000u)) {
                const float4* rp = reinterpret_cast<const float4*>(g_rec + (size_t)((int)(e2[b] & 0x7fffffffu) * LRT_LEAF + c) * LRT_REC_FLOATS);
                q0[b] = rp[0]; q1[b] = rp[1]; q2[b] = rp[2]; q3[b] = rp[3];
            } else if (has2[b]) {
                const float4* nd = reinterpret_cast<const float4*>(g_naos + (size_t)e2[b] * LRT_NODE_FLOATS) + 2 * c;
                q0[b] = nd[0]; q1[b] = nd[1];
            }
        }
#pragma unroll
        for (int b = 0; b < NEAR_NB; b++) {
            if (take <= 8 * b) break;                                         // (uniform)
            const bool has = has2[b]; const unsigned e = e2[b];
            bool hitq = false, hitn = false; float t = 0.f; int slot = 0; unsigned ent = 0u;
            if (has && (e & 0x80000000u)) {
                slot = (int)(e & 0x7fffffffu) * LRT_LEAF + c;
                const float rc[LRT_REC_FLOATS] = {q0[b].x, q0[b].y, q0[b].z, q0[b].w, q1[b].x, q1[b].y, q1[b].z, q1[b].w, q2[b].x, q2[b].y, q2[b].z, q2[b].w, q3[b].x, q3[b].y, q3[b].z, q3[b].w};
                if (rc[7] > 0.f) {
                    const float cx = rc[4] - o[0], cy = rc[5] - o[1], cz = rc[6] - o[2];
                    t = (rc[0] * cx + rc[1] * cy + rc[2] * cz) / (rc[0] * d[0] + rc[1] * d[1] + rc[2] * d[2]);
                    const float px = t * d[0] - cx, py = t * d[1] - cy, pz = t * d[2] - cz;
                    const float u = rc[8] * px + rc[9] * py + rc[10] * pz, v = rc[12] * px + rc[13] * py + rc[14] * pz;
                    hitq = (t > 0.f) && (t < 1e16f) && (fabsf(u) <= rc[7]) && (fabsf(v) <= rc[7]) && (t >= b_lo) && (t < b_hi);
                }
            } else if (has) {
                const float4 A = q0[b], B = q1[b];
                const float tx0 = (A.x - o[0]) * inv[0], tx1 = (A.y - o[0]) * inv[0], ty0 = (A.z - o[1]) * inv[1], ty1 = (A.w - o[1]) * inv[1];
                const float tz0 = (B.x - o[2]) * inv[2], tz1 = (B.y - o[2]) * inv[2];
                const float tn = fmaxf(fmaxf(fminf(tx0, tx1), fminf(ty0, ty1)), fminf(tz0, tz1));
                const float tf = fminf(fminf(fmaxf(tx0, tx1), fmaxf(ty0, ty1)), fmaxf(tz0, tz1));
                const bool in_ = (A.x < LRT_EMPTY) && (tf >= fmaxf(tn, 0.f));
                hitn = in_ && (tf >= b_lo) && (tn < b_hi);
                beyond = beyond | (in_ && (tf >= b_hi));
                ent = (unsigned)__float_as_int(B.z) | ((__float_as_int(B.w) & 1) ? 0x80000000u : 0u);
            }
            const unsigned long long mq = __ballot(hitq), mn = __ballot(hitn);
            const int k = n + __popcll(mq & below);
            if (hitq && st.n + k < NEAR_CAP) { s_t[k] = t; s_s[k] = slot; }
            n += __popcll(mq);
            if (st.n + n > NEAR_CAP) ovf = true;
            if (sp + __popcll(mn) > NEAR_STACK) ovf = true;
            else { if (hitn) s_stack[sp + __popcll(mn & below)] = ent; sp += __popcll(mn); }
        }
    }
    if (ovf) { st.ovf = 1; st.more = 0; return st; }
    // ---- rank sort of the new hits by (t, gidx), behind the stream
    for (int i = lane; i < n; i += 64) {
        const float ti = s_t[i];
        int rk = 0, eq = 0;
        for (int k = 0; k < n; k++) { const float tk = s_t[k]; rk += (tk < ti) ? 1 : 0; eq += (tk == ti) ? 1 : 0; }
        if (eq > 1) {                                                          // equal depths (rare): (t, gidx) order, the Gaussians from the hits' records
            const int gi = __float_as_int(g_rec[(size_t)s_s[i] * LRT_REC_FLOATS + 11]);
            for (int k = 0; k < n; k++)
                if (s_t[k] == ti && __float_as_int(g_rec[(size_t)s_s[k] * LRT_REC_FLOATS + 11]) < gi) rk++;
        }
        s_ts[st.n + rk] = ti; s_ss[st.n + rk] = s_s[i];
    }
    st.n += n; st.more = __any(beyond) ? 1 : 0;
    return st;
}

__device__ __forceinline__ int near_rdli(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ void near_loop_wave(const TraceParams& p, const float* __restrict__ g_rec, const float* __restrict__ g_naos, NearLds& L, int r, int lane,
                                               const float* o, const float* d, const float* inv)
{
    const float* const s_ts = L.ts; const int* const s_ss = L.ss;
    float bt = 1e16f; int bs = -1;                                    // slot `lane` of the K-buffer (lanes >= 16: unused copies that never take part)
    float T = 1.f, test_T = 1.f, dpt = 0.f, pdpt = 0.f, Dd = 0.f, Wt = 0.f;
    int last_g = -1, n_rec = 0, first = 0;
    const bool in16 = lane < LRT_CHUNK;
    // the stream of the ray's hits in ascending depth, collected slab by slab when the loop runs out of candidates (see near_replay)
    NearSt st = {0, 0.f, 1, 0};
    float next_hi = NEAR_SLAB0; int refills = 0;
    auto ensure = [&](int k) {                                        // candidate k exists, or the scene holds no more
        while (k >= st.n && st.more && !st.ovf) {
            const float b_lo = st.b_hi;
            st.b_hi = refills >= 5 ? 3.0e38f : next_hi; next_hi *= 4.f; refills++;
            st = near_collect(g_rec, g_naos, L, o, d, inv, lane, st, b_lo);
        }
    };
    for (int chunk = 0; chunk < 4096; chunk++) {
        unsigned cnt = 0;
        for (;;) {                                                                   // hits at or before the moved origin (tmin = 0)
            ensure(first);
            if (first < st.n && !(s_ts[first] - pdpt > 0.f)) first++; else break;
        }
        for (int k = first; ; k++) {                                             // traceStep + __anyhit__ot (forward.cu:312-356), ascending stream
            ensure(k);
            if (k >= st.n) break;
            const float ct = s_ts[k] - pdpt; const int cs = s_ss[k];
            if (!(ct < rdl(bt, LRT_CHUNK - 1))) break;                           // nothing later can enter either
            cnt++;
            const int pos = __popcll(__ballot(in16 && !(bt > ct)));              // slots that stay in front of the candidate
            // (the value of the previous lane over the DPP network -- wave_shr:1, lane 0 keeps its own: __shfl_up is a round trip through the LDS crossbar, twice per candidate)
            const float ut = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(bt), __float_as_int(bt), 0x138, 0xf, 0xf, false));
            const int us = __builtin_amdgcn_update_dpp(bs, bs, 0x138, 0xf, 0xf, false);
            if (in16 && lane >= pos) { bt = lane == pos ? ct : ut; bs = lane == pos ? cs : us; }
        }
        if (st.ovf) { if (lane == 0 && p.err_flag) atomicOr(p.err_flag, 1); return; }     // > 1024 quads on a near ray: reported like a list overflow
        // ---- all 16 slots at once: depth, record, alpha
        const float dp = bt + pdpt;
        const bool mine = in16 && (unsigned)lane < cnt;
        const bool near_l = dp < LRT_T_NEAR;
        int g_l = -1; float ao_l = 0.f; bool skip_l = false;
        if (mine && !near_l && bs >= 0) {
            const float4* rp = reinterpret_cast<const float4*>(g_rec + (size_t)bs * LRT_REC_FLOATS);
            const float4 r0 = rp[0], r1 = rp[1], r2 = rp[2], r3 = rp[3];
            const float rc[LRT_REC_FLOATS] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, r3.x, r3.y, r3.z, r3.w};
            g_l = __float_as_int(rc[11]);
            ao_l = near_alpha(rc, o, d, dp, skip_l);
        }
        // ---- the decisions, slot by slot (uniform: every lane walks the same values)
        bool brk = false;
        for (int i = 0; i < LRT_CHUNK && !brk; i++) {
            if ((unsigned)i >= cnt) break;
            dpt = rdl(dp, i);
            if (near_rdli(near_l ? 1 : 0, i)) continue;                               // forward.cu:214: the slot is NOT cleared
            const int slot = near_rdli(bs, i);
            if (lane == i) { bt = 1e16f; bs = -1; }
            if (slot < 0) { last_g = 0; continue; }                              // a cleared slot inside cnt: gidx 0 at depth 1e16 (forward.cu:218-222)
            const int g = near_rdli(g_l, i);
            if (g == last_g) continue;
            last_g = g;
            if (near_rdli(skip_l ? 1 : 0, i)) continue;
            const float ao = rdl(ao_l, i);
            const float alpha = fminf(LRT_ALPHA_MAX, ao);
            if (alpha < LRT_ALPHA_MIN) continue;
            test_T = T * (1.f - alpha);
            if (test_T < LRT_T_STOP) { brk = true; break; }
            const float w = alpha * T;
            Dd += w * dpt; Wt += w;
            if (lane == 0) {
                if (p.accum) unsafeAtomicAdd(p.accum + g, w);                    // (null: option deferred_accum)
                if (p.hit_t) {
                    if (n_rec < p.hit_cap) {
                        const size_t id = (size_t)r * p.hit_cap + n_rec;
                        p.hit_t[id] = dpt; p.hit_g[id] = g;
                        if (p.hit_wa) p.hit_wa[id] = make_float2(w, ao);
                    } else if (p.ovf_list) {
                        const unsigned ix = atomicAdd(p.ovf_count, 1u);
                        if (ix < p.ovf_cap) p.ovf_list[ix] = make_float4(__int_as_float(r), __int_as_float(g), w, 0.f);
                        else if (p.err_flag) atomicOr(p.err_flag, 4);
                    }
                }
            }
            if (p.hit_t) n_rec++;
            T = test_T;
        }
        if (test_T < LRT_T_STOP || cnt < (unsigned)LRT_CHUNK) break;
        pdpt = dpt + LRT_STEP_EPS;
    }
    if (lane != 0) return;
    float* op_ = p.out9 + LRT_NCH * (size_t)r;
    op_[3] = Dd; op_[4] = Wt; op_[5] = 0.f; op_[6] = 0.f; op_[7] = 0.f; op_[8] = T;       // (colours: the deferred pass)
    if (p.hit_t) {
        p.hit_n[r] = min(n_rec, p.hit_cap); if (n_rec > p.hit_cap) atomicOr(p.hit_ovf, 1);
        if (p.hit_count) atomicAdd(p.hit_count, (unsigned)min(n_rec, p.hit_cap));
    }
}

// One ray, one wave.  BWD = false: the forward (outputs, accum, hit record).  BWD = true: the re-tracing backward's counterpart -- the same
// loop, and every composited hit's gradient goes out through bwd_hit's atomics (backward.cu:524-533 has the same stale-slot order as
// the forward).
template <bool BWD>
__device__ __forceinline__ void near_replay(const TraceParams& p, const float* __restrict__ g_rec, const float* __restrict__ g_naos, int r, int defer, int lane, NearLds& L)
{
    float* const s_t = L.t; float* const s_ts = L.ts; int* const s_s = L.s; int* const s_ss = L.ss; unsigned* const s_stack = L.stack;
    const unsigned long long below = (1ull << lane) - 1ull;
    {
        float o[3], d[3], inv[3];
        for (int i = 0; i < 3; i++) {
            o[i] = p.ray_o[3 * (size_t)r + i]; d[i] = p.ray_d[3 * (size_t)r + i];
            inv[i] = (fabsf(d[i]) < 1e-30f) ? copysignf(1e30f, d[i]) : 1.0f / d[i];
        }
        // The production forward (the 16-slot window across 16 lanes) collects the ray's hits LAZILY, depth slab by depth slab, as its loop asks for them: a ray
        // that ends at T < 1e-4 after a few metres never walks the scene behind (round 6: the exhaustive walk was half of the replay's time).  The literal
        // one-lane consumers below (re-tracing backward, non-deferred forward) take everything at once.
        if (!BWD && defer) { near_loop_wave(p, g_rec, g_naos, L, r, lane, o, d, inv); return; }
        NearSt st = {0, 3.0e38f, 0, 0};
        st = near_collect(g_rec, g_naos, L, o, d, inv, lane, st, 0.f);
        if (st.ovf) { if (lane == 0 && p.err_flag) atomicOr(p.err_flag, 1); return; }     // > 1024 quads on a near ray: reported like a list overflow
        const int n = st.n;
        // (one wave: LDS operations are in order, no barrier needed)
        if (lane != 0) return;
        // ---- the reference's raygen loop (forward.cu:195-292), any-hit fed in ascending t
        float bt[LRT_CHUNK]; int bs[LRT_CHUNK];
        for (int i = 0; i < LRT_CHUNK; i++) { bt[i] = 1e16f; bs[i] = -1; }
        float T = 1.f, test_T = 1.f, dpt = 0.f, pdpt = 0.f, C0 = 0.f, C1 = 0.f, C2 = 0.f, Dd = 0.f, Wt = 0.f;
        int last_g = -1, n_rec = 0, first = 0;
        float b[16];
        if (!defer || BWD) lrt_sh_basis(p.deg, d, b);
        float N0 = 0.f, N1 = 0.f, N2 = 0.f, go[3] = {0.f, 0.f, 0.f}, gd[3] = {0.f, 0.f, 0.f};
        float dL[LRT_NCH], fin[LRT_NCH], dL_dbg = 0.f;
        if (BWD) {
            for (int i = 0; i < LRT_NCH; i++) { dL[i] = p.dL_dout[LRT_NCH * (size_t)r + i]; fin[i] = p.out9_in[LRT_NCH * (size_t)r + i]; }
            dL_dbg = dL[0] * p.bg[0] + dL[1] * p.bg[1] + dL[2] * p.bg[2];
        }
        for (int chunk = 0; chunk < 4096; chunk++) {
            unsigned cnt = 0;
            while (first < n && !(s_ts[first] - pdpt > 0.f)) first++;              // hits at or before the moved origin (tmin = 0)
            for (int k = first; k < n; k++) {                                        // traceStep + __anyhit__ot (forward.cu:312-356)
                float ct = s_ts[k] - pdpt; int cs = s_ss[k];
                if (!(ct < bt[LRT_CHUNK - 1])) break;                                // ascending stream: nothing later can enter either
                cnt++;
                for (int i = 0; i < LRT_CHUNK; i++)
                    if (bt[i] > ct) { const float tt = bt[i]; const int ts_ = bs[i]; bt[i] = ct; bs[i] = cs; ct = tt; cs = ts_; }
            }
            bool brk = false;
            for (int i = 0; i < LRT_CHUNK && !brk; i++) {
                if ((unsigned)i >= cnt) break;
                const int slot = bs[i];
                dpt = bt[i] + pdpt;
                if (dpt < LRT_T_NEAR) continue;                                      // forward.cu:214: the slot is NOT cleared
                bt[i] = 1e16f; bs[i] = -1;
                if (slot < 0) { last_g = 0; continue; }                              // a cleared slot inside cnt: the reference reads idx 0 -> gidx 0 at depth 1e16, not composited, but last_gidx becomes 0 (forward.cu:218-222)
                const float* rc = g_rec + (size_t)slot * LRT_REC_FLOATS;
                const int g = __float_as_int(rc[11]);
                if (g == last_g) continue;
                last_g = g;
                bool skip;
                const float ao = near_alpha(rc, o, d, dpt, skip);
                if (skip) continue;
                const float alpha = fminf(LRT_ALPHA_MAX, ao);
                if (alpha < LRT_ALPHA_MIN) continue;
                test_T = T * (1.f - alpha);
                if (test_T < LRT_T_STOP) { brk = true; break; }
                if (BWD) {                                                           // backward.cu:538-676 on this hit, at the depth the forward used
                    RayAcc a = {T, C0, C1, C2, Dd, Wt, N0, N1, N2, {go[0], go[1], go[2]}, {gd[0], gd[1], gd[2]}};
                    bwd_hit<false, true>(p, o, d, b, p.nsh, dL, fin, dL_dbg, dpt, g, 0.f, a);
                    C0 = a.C0; C1 = a.C1; C2 = a.C2; Dd = a.Dd; N0 = a.N0; N1 = a.N1; N2 = a.N2;
                    for (int i2 = 0; i2 < 3; i2++) { go[i2] = a.go[i2]; gd[i2] = a.gd[i2]; }
                    T = test_T;
                    continue;
                }
                const float w = alpha * T;
                if (!defer) { float c0, c1, c2; bool cl0; sh_colour(p, g, b, p.nsh, c0, c1, c2, cl0); C0 += w * c0; C1 += w * c1; C2 += w * c2; }
                Dd += w * dpt; Wt += w;
                if (p.accum) unsafeAtomicAdd(p.accum + g, w);                        // (null: option deferred_accum)
                if (p.hit_t) {
                    if (n_rec < p.hit_cap) {
                        const size_t id = (size_t)r * p.hit_cap + n_rec;
                        p.hit_t[id] = dpt; p.hit_g[id] = g;
                        if (p.hit_wa) p.hit_wa[id] = make_float2(w, ao);
                    } else if (defer && p.ovf_list) {
                        const unsigned ix = atomicAdd(p.ovf_count, 1u);
                        if (ix < p.ovf_cap) p.ovf_list[ix] = make_float4(__int_as_float(r), __int_as_float(g), w, 0.f);
                        else if (p.err_flag) atomicOr(p.err_flag, 4);
                    }
                    n_rec++;
                }
                T = test_T;
            }
            if (test_T < LRT_T_STOP || cnt < (unsigned)LRT_CHUNK) break;
            pdpt = dpt + LRT_STEP_EPS;
        }
        if (BWD) { if (p.d_ray_o) store_ray_grad(p, (size_t)r, go, gd); return; }
        float* op_ = p.out9 + LRT_NCH * (size_t)r;
        if (!defer) { op_[0] = C0 + T * p.bg[0]; op_[1] = C1 + T * p.bg[1]; op_[2] = C2 + T * p.bg[2]; }
        op_[3] = Dd; op_[4] = Wt; op_[5] = 0.f; op_[6] = 0.f; op_[7] = 0.f; op_[8] = T;
        if (p.hit_t) {
            p.hit_n[r] = min(n_rec, p.hit_cap); if (n_rec > p.hit_cap) atomicOr(p.hit_ovf, 1);
            if (p.hit_count) atomicAdd(p.hit_count, (unsigned)min(n_rec, p.hit_cap));
        }
    }
}

__global__ void __launch_bounds__(64) k_fwd_near(const TraceParams p, const float* __restrict__ g_rec, const float* __restrict__ g_naos, int defer)
{
    __shared__ NearLds L;
    const unsigned n_near = min(*p.near_count, (unsigned)p.H * (unsigned)p.W);
    if (n_near == 0u) return;
    if (!p.near_done) { for (unsigned qi = blockIdx.x; qi < n_near; qi += gridDim.x) near_replay<false>(p, g_rec, g_naos, p.near_list[qi], defer, (int)threadIdx.x, L); return; }
    // rays by ticket (round 6): their costs differ several-fold -- a fixed share per wave ends with the unluckiest wave
    for (unsigned qi = blockIdx.x; qi < n_near; ) {
        near_replay<false>(p, g_rec, g_naos, p.near_list[qi], defer, (int)threadIdx.x, L);
        unsigned nx = 0u;
        if (threadIdx.x == 0) nx = atomicAdd(p.near_done, 1u);
        qi = gridDim.x + (unsigned)__builtin_amdgcn_readfirstlane((int)nx);
    }
}
