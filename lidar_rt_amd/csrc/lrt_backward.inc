// lrt_backward.inc -- backward kernels on the forward's hit record: replay with atomics, per-ray preparation,
// sorted segmented reductions (included by lrt_kernels.hip after TraceParams and the wave helpers).

// Device-side decision of the stream-ordered backward (see lrt_backward): true = this kernel has nothing to do.
__device__ __forceinline__ bool bwd_guard_skips(const TraceParams& p)
{
    if (p.guard == 0) return false;
    const bool bad = (*p.hit_ovf != 0) || (*p.n_hits_dev > p.n_spec);
    return (p.guard == 1) == bad;
}

#define BK_RB 4                          // row blocks of the count matrix scan (k_bk_scan)

// Ray i of ray group g (k_bk_count and k_bwd_prep2 must agree).  bk_cw > 0: a group is a block of bk_cw image COLUMNS over ALL rows -- every group holds
// the same mix of beams.  Measured on S1M: the upper 16 beams composite 57 hits per ray, the lower 32 beams 16; groups of 256 consecutive rays (an eighth of
// one beam) held up to 2.3 x the mean number of hits, and both kernels run ONE workgroup per group, all resident at once: they lasted as long as their
// heaviest group.  bk_cw = 0: bk_rpg consecutive rays (the cross-check library's k_bwd_prep; images with more rows than a workgroup should walk).
__device__ __forceinline__ bool bk_group_ray(const TraceParams& p, unsigned g, unsigned i, unsigned* r)
{
    if (p.bk_cw) {
        const unsigned cw = (unsigned)p.bk_cw, h = i / cw, w = g * cw + (i - h * cw);
        *r = h * (unsigned)p.W + w;
        return i < (unsigned)p.bk_rpg && w < (unsigned)p.W && h < (unsigned)p.H;
    }
    *r = g * (unsigned)p.bk_rpg + i;
    return i < (unsigned)p.bk_rpg && *r < (unsigned)p.hw;
}
// Bucketed backward: zero the gradient rows of the 2^bk_shift Gaussians of bucket b (all five tables), by `nt` threads.
__device__ __forceinline__ void bk_zero_rows(const TraceParams& p, int b, int tid, int nt)
{
    const int Gb = 1 << p.bk_shift;
    const size_t g0 = (size_t)b * Gb;
    const int ng = (int)min((size_t)Gb, (size_t)p.P - g0);
    const int M3 = 3 * p.M;
    for (int i = tid; i < ng * 3; i += nt) p.d_means[g0 * 3 + i] = 0.f;
    for (int i = tid; i < ng * 2; i += nt) p.d_scales[g0 * 2 + i] = 0.f;
    for (int i = tid; i < ng * 4; i += nt) p.d_rots[g0 * 4 + i] = 0.f;
    for (int i = tid; i < ng; i += nt) p.d_opac[g0 + i] = 0.f;
    for (int i = tid; i < ng * M3; i += nt) p.d_shs[g0 * M3 + i] = 0.f;
    if (p.accum) for (int i = tid; i < ng; i += nt) p.accum[g0 + i] = 0.f;      // option deferred_accum: the backward owns the column
}

// n floats at p <- 0 by `nthr` threads (thread `tid`): whole 16-byte stores between an unaligned head and tail
__device__ __forceinline__ void bk_zero_span(float* p, size_t n, size_t tid, size_t nthr)
{
    if (!p || n == 0) return;
    const size_t head = min(n, (size_t)((16u - (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) / 4u);
    float4* p4 = reinterpret_cast<float4*>(p + head);
    const size_t n4 = (n - head) / 4u;
    for (size_t i = tid; i < n4; i += nthr) p4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tid < head) p[tid] = 0.f;
    const size_t tail0 = head + 4u * n4;
    if (tid < n - tail0) p[tail0 + tid] = 0.f;
}

// Bucketed backward, prologue of the per-ray replay (workgroups of 1024 threads, one per ray group): the LDS cursor of bucket b starts
// at  base[b] + (hits of the earlier groups in b)  with base[] = exclusive prefix of the buckets' totals.  Every workgroup scans the
// totals for itself (round 4: the one-workgroup launch k_bk_base between k_bk_scan and this kernel is gone; <= 16 consecutive buckets
// per thread, wave scans, one barrier pair) and workgroup 0 stores base[0 .. nb] for the kernels behind (k_bk_sort, k_bwd_reduce4).
__device__ __forceinline__ void bk_setup_cursors(const TraceParams& p, unsigned* s_cur, unsigned* s_h /* [16] */)
{
    const int nb = p.bk_nb, per = (nb + 1023) / 1024;           // <= 16 (BK_MAX_NB = 16384)
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int b0 = tid * per, b1 = min(b0 + per, nb);
    const unsigned* row = p.bk_M + (size_t)blockIdx.x * nb;
    const int rbg = (p.bk_ng + BK_RB - 1) / BK_RB, rb = (int)blockIdx.x / rbg;      // the row block of k_bk_scan this group lies in
    // two passes over this thread's buckets (the second one hits the caches) instead of per-bucket arrays: the caller is capped at 64 VGPRs
    unsigned hs = 0u;
    for (int b = b0; b < b1; ++b)
        for (int y = 0; y < BK_RB; ++y) hs += p.bk_aux[(size_t)y * nb + b];
    unsigned incl = hs;
    for (int o = 1; o < 64; o <<= 1) { const unsigned v = __shfl_up(incl, o); if (lane >= o) incl += v; }
    if (lane == 63) s_h[wv] = incl;
    __syncthreads();
    unsigned bef = 0u, all = 0u;
    for (int k = 0; k < 16; ++k) { const unsigned v = s_h[k]; if (k < wv) bef += v; all += v; }
    unsigned hrun = bef + incl - hs;
    for (int b = b0; b < b1; ++b) {
        unsigned tot = 0u, before = row[b];
        for (int y = 0; y < BK_RB; ++y) { const unsigned v = p.bk_aux[(size_t)y * nb + b]; tot += v; before += (y < rb) ? v : 0u; }
        s_cur[b] = hrun + before;
        if (blockIdx.x == 0) p.bk_base[b] = hrun;
        hrun += tot;
    }
    if (blockIdx.x == 0 && tid == 1023) p.bk_base[nb] = all;
    __syncthreads();
}

#ifdef LRT_LEGACY      // cross-check build only (bwd_mode 1 / 2, forwards without deferred colour): see lidar_rt_amd/build.py
// Backward by REPLAY of the hit record the forward wrote (no traversal; the reference re-traces, backward.cu:513).
// One lane per ray, same 64-ray tiles as the forward so that neighbouring lanes scatter into neighbouring Gaussians.
template <bool SCATTER>
__global__ void __launch_bounds__(256) k_bwd_replay(const TraceParams p)
{
    const int lane = threadIdx.x & 63;
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= p.n_tiles) return;
    const int TWm = (1 << p.tw_log2) - 1, TH = 64 >> p.tw_log2;
    const int ty = tile % p.tiles_y, tx = tile / p.tiles_y;
    const int h = ty * TH + (lane >> p.tw_log2), w = (tx << p.tw_log2) + (lane & TWm);
    const bool valid = (h < p.H) && (w < p.W);
    const size_t r = valid ? ((size_t)h * p.W + w) : 0;
    float o[3], d[3];
    for (int i = 0; i < 3; i++) { o[i] = p.ray_o[3 * r + i]; d[i] = p.ray_d[3 * r + i]; }
    float b[16];
    lrt_sh_basis(p.deg, d, b);
    float dL[LRT_NCH], fin[LRT_NCH];
    for (int i = 0; i < LRT_NCH; i++) { dL[i] = p.dL_dout[LRT_NCH * r + i]; fin[i] = p.out9_in[LRT_NCH * r + i]; }
    const float dL_dbg = dL[0] * p.bg[0] + dL[1] * p.bg[1] + dL[2] * p.bg[2];
    RayAcc a = {1.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (!SCATTER && valid) {
        float4* rp = p.ray_pk + 4 * r;
        rp[0] = make_float4(o[0], o[1], o[2], dL[3]); rp[1] = make_float4(d[0], d[1], d[2], 0.f);
        rp[2] = make_float4(dL[0], dL[1], dL[2], 0.f); rp[3] = make_float4(dL[5], dL[6], dL[7], 0.f);
    }
    const int n = valid ? min(p.hit_n[r], p.hit_cap) : 0;
    for (int j = 0; __any(j < n); ++j) {
        if (j < n) {
            const size_t id = r * (size_t)p.hit_cap + j;
            const float t = p.hit_t[id];
            const int g = p.hit_g[id];
            bwd_hit<false, SCATTER>(p, o, d, b, p.nsh, dL, fin, dL_dbg, t, g, 0.f, a, id);
            if (!SCATTER) {                          // dense (gidx, id) key list for the sort: slot = exclusive_scan(hit_n)[r] + j
                const unsigned slot = p.hit_off[r] + (unsigned)j;
                if (slot < p.key_cap) p.hit_keys[slot] = ((unsigned long long)(unsigned)g << p.id_bits) | (unsigned long long)id;
            }
        }
    }
}

// Replay for the sorted-reduction backward, ONE RAY PER WAVE: lane j takes the j-th composited hit of the ray (the
// record is ray-major, so the loads are coalesced), the transmittance is a wave prefix product and the running sums
// of the reference's sequential loop (C, D, N "so far", backward.cu:576-604) are wave prefix sums.  131k independent
// ray tasks instead of 2k waves each walking 64 rays hit by hit.  Writes (t, dL/dalpha, +-w) per hit, the dense
// (gidx, id) key list and the per-ray pack.
// FAST: the deferred-colour forward left (weight, op*G) in hit_wa and k_fwd_colour left the hit's colour in hit_pk, so the
// per-hit gathers of the Gaussian (40 B) and of its SH table (192 B) are not repeated here.
// BUCKET (bwd_mode 3, lrt_bucket.inc): a workgroup of 16 waves takes one GROUP of rays (the rows of the count matrix); instead of
// (t, dL/dalpha, +-w) at the hit's own place plus a sort key, the hit's 16-byte record goes to the next free slot of its Gaussian's
// bucket -- the cursors of the group live in LDS, initialised from the scanned count matrix.
template <bool FAST, bool BUCKET>
__global__ void __launch_bounds__(BUCKET ? 1024 : 64, BUCKET ? (FAST ? 8 : 4) : 1) k_bwd_prep(const TraceParams p)
{
    extern __shared__ unsigned s_cur[];
    const int lane = threadIdx.x & 63;
    const int nsh = p.nsh;
    const float bg0 = p.bg[0], bg1 = p.bg[1], bg2 = p.bg[2];
    if (bwd_guard_skips(p)) return;
    unsigned r_begin, r_end, r_step;
    if (BUCKET) {
        __shared__ unsigned s_h16[16];
        bk_setup_cursors(p, s_cur, s_h16);
        r_begin = blockIdx.x * (unsigned)p.bk_rpg + (threadIdx.x >> 6); r_end = min((blockIdx.x + 1u) * (unsigned)p.bk_rpg, (unsigned)p.hw); r_step = blockDim.x >> 6;
    } else {
        if (p.n_hits_dev) {          // the sort covers n_spec >= n_hits keys: the tail gets keys that sort last and that the reduction ignores
            const unsigned nh = *p.n_hits_dev;
            for (unsigned long long i = (unsigned long long)nh + blockIdx.x * 64ull + lane; i < p.n_spec; i += (unsigned long long)gridDim.x * 64ull) p.hit_keys[i] = ~0ull;
        }
        r_begin = blockIdx.x; r_end = (unsigned)p.hw; r_step = gridDim.x;
    }
    for (unsigned r = r_begin; r < r_end; r += r_step) {
        const int n = min(p.hit_n[r], p.hit_cap);
        if (n == 0) continue;
        float o[3], d[3], dL[LRT_NCH], fin[LRT_NCH];
        for (int i = 0; i < 3; i++) { o[i] = p.ray_o[3 * (size_t)r + i]; d[i] = p.ray_d[3 * (size_t)r + i]; }
        for (int i = 0; i < LRT_NCH; i++) { dL[i] = p.dL_dout[LRT_NCH * (size_t)r + i]; fin[i] = p.out9_in[LRT_NCH * (size_t)r + i]; }
        if (lane < 4) {
            const float4 v = lane == 0 ? make_float4(o[0], o[1], o[2], dL[3]) : (lane == 1 ? make_float4(d[0], d[1], d[2], 0.f) :
                             (lane == 2 ? make_float4(dL[0], dL[1], dL[2], 0.f) : make_float4(dL[5], dL[6], dL[7], 0.f)));
            p.ray_pk[4 * (size_t)r + lane] = v;
        }
        const float dL_dbg = dL[0] * bg0 + dL[1] * bg1 + dL[2] * bg2;
        const bool need_n = (dL[5] != 0.f) || (dL[6] != 0.f) || (dL[7] != 0.f);
        float b[16];
        lrt_sh_basis(p.deg, d, b);
        const unsigned off = BUCKET ? 0u : p.hit_off[r];
        float T_run = 1.f, rC0 = 0.f, rC1 = 0.f, rC2 = 0.f, rD = 0.f, rN0 = 0.f, rN1 = 0.f, rN2 = 0.f;
        for (int cb = 0; cb < n; cb += 64) {
            const int j = cb + lane;
            const bool live = j < n;
            const size_t id = (size_t)r * p.hit_cap + (live ? j : cb);
            const float t = p.hit_t[id];
            const int g = p.hit_g[id];
            float c0, c1, c2, ao, n0 = 0.f, n1 = 0.f, n2 = 0.f; bool cl0;
            if (FAST) {
                const float4 cc = p.hit_pk[id];                      // written by k_fwd_colour, overwritten below by the same lane
                c0 = cc.x; c1 = cc.y; c2 = cc.z; cl0 = cc.w < 0.f;
                ao = fabsf(cc.w);                                    // op * G, the clamp flag as its sign (k_fwd_colour)
                if (need_n) {                                        // normals only matter for upstream gradients on channels 5..7 (D3)
                    const float q[4] = {p.rots[4 * (size_t)g], p.rots[4 * (size_t)g + 1], p.rots[4 * (size_t)g + 2], p.rots[4 * (size_t)g + 3]};
                    float R[9];
                    lrt_quat_to_R(q, R);
                    n0 = R[2]; n1 = R[5]; n2 = R[8];
                }
            } else {
                const float mu[3] = {p.means[3 * (size_t)g], p.means[3 * (size_t)g + 1], p.means[3 * (size_t)g + 2]};
                const float sc[2] = {p.scales[2 * (size_t)g], p.scales[2 * (size_t)g + 1]};
                const float q[4] = {p.rots[4 * (size_t)g], p.rots[4 * (size_t)g + 1], p.rots[4 * (size_t)g + 2], p.rots[4 * (size_t)g + 3]};
                sh_colour(p, g, b, nsh, c0, c1, c2, cl0);
                LrtHitGeom hg;
                lrt_hit_geom(o, d, t, mu, sc, q, p.mod, &hg);
                ao = p.opac[g] * hg.G;
                n0 = hg.R[2]; n1 = hg.R[5]; n2 = hg.R[8];
            }
            const float alpha = fminf(LRT_ALPHA_MAX, ao);
            const float incl = wave_incl_prod(live ? (1.f - alpha) : 1.f);
            float excl = __shfl_up(incl, 1);
            if (lane == 0) excl = 1.f;
            const float Tk = T_run * excl;
            const float wgt = live ? alpha * Tk : 0.f;
            const float sC0 = rC0 + wave_incl_sum(wgt * c0), sC1 = rC1 + wave_incl_sum(wgt * c1), sC2 = rC2 + wave_incl_sum(wgt * c2);
            const float sD = rD + wave_incl_sum(wgt * t);
            float sN0 = rN0, sN1 = rN1, sN2 = rN2;                   // normals: only with upstream gradients on channels 5..7 (wave-uniform)
            if (need_n) { sN0 += wave_incl_sum(wgt * n0); sN1 += wave_incl_sum(wgt * n1); sN2 += wave_incl_sum(wgt * n2); }
            const float i1a = 1.0f / (1.0f - alpha);
            float dLa = dL[0] * (Tk * c0 - (fin[0] - sC0) * i1a) + dL[1] * (Tk * c1 - (fin[1] - sC1) * i1a) +
                        dL[2] * (Tk * c2 - (fin[2] - sC2) * i1a);
            dLa += dL_dbg * (-fin[8] * i1a);                        // D1 (backward.cu:595-598)
            dLa += dL[3] * (Tk * t - (fin[3] - sD) * i1a);
            if (need_n) dLa += dL[5] * (Tk * n0 - (fin[5] - sN0) * i1a) + dL[6] * (Tk * n1 - (fin[6] - sN1) * i1a) +
                               dL[7] * (Tk * n2 - (fin[7] - sN2) * i1a);        // D3
            dLa *= (ao > LRT_ALPHA_MAX) ? 0.f : 1.f;                // backward.cu:607-608
            if (live && BUCKET) {
                const unsigned slot = atomicAdd(&s_cur[(unsigned)g >> p.bk_shift], 1u);
                if (slot < p.rec_cap)
                    p.brec[slot] = make_uint4((r << p.bk_shift) | ((unsigned)g & ((1u << p.bk_shift) - 1u)), __float_as_uint(t), __float_as_uint(dLa), __float_as_uint(cl0 ? -wgt : wgt));
            } else if (live) {
                if (p.accum) unsafeAtomicAdd(p.accum + g, wgt);      // option deferred_accum on the sorted path: one atomic per hit, as the forward would have issued
                p.hit_pk[id] = make_float4(t, dLa, cl0 ? -wgt : wgt, 0.f);
                const unsigned slot = off + (unsigned)j;
                if (slot < p.key_cap) p.hit_keys[slot] = ((unsigned long long)(unsigned)g << p.id_bits) | (unsigned long long)id;
            }
            // carries for rays with more than 64 composited hits
            T_run *= rdl(incl, 63);
            rC0 = rdl(sC0, 63); rC1 = rdl(sC1, 63); rC2 = rdl(sC2, 63); rD = rdl(sD, 63);
            if (need_n) { rN0 = rdl(sN0, 63); rN1 = rdl(sN1, 63); rN2 = rdl(sN2, 63); }
        }
    }
}

#endif  // LRT_LEGACY

// k_bwd_prep<true, true> with TWO rays per wave (the bucketed backward behind a deferred-colour forward, i.e. the default training path):
// a ray composites 30 hits on average, so a wave per ray left half of the lanes idle and every wave walked 16 rays one memory round trip
// after the other.  Lanes 0..31 take ray 2k, lanes 32..63 ray 2k + 1 of the group; the prefix product / sums run inside each half
// (the wave scans without their last DPP step), a ray with more than 32 hits loops with carries taken from lane 31 / 63.
//
// MODE 1 (lrt_backward_rays, one extra launch behind MODE 0): the same replay of the same record with the same dL/dalpha per hit, but instead
// of the hit's bucket record it forms the hit's share of the RAY's gradient (lrt_hit_ray_backward on the Gaussian's geometry, and the colour
// term dL/dbasis from its SH row), sums it inside the half-wave that owns the ray and stores 6 floats per ray.  No cursors, no clearing, no
// LDS; a register budget of its own (MODE 0 stays at its 64).
template <int MODE>
__global__ void __launch_bounds__(1024, MODE == 0 ? 8 : 1) k_bwd_prep2(const TraceParams p)
{
    extern __shared__ unsigned s_cur[];
    const int lane = threadIdx.x & 63, hl = lane & 31, half = lane >> 5;
    const float bg0 = p.bg[0], bg1 = p.bg[1], bg2 = p.bg[2];
    if (bwd_guard_skips(p)) return;
    if (MODE == 0 && p.zero_in_prep) {
        const size_t tid_ = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nthr_ = (size_t)gridDim.x * blockDim.x, P_ = (size_t)p.P;
        // Round 6: the gradient tensors are cleared HERE, whole, by streaming 16-byte stores that this latency-bound kernel (its waves wait 70 % of
        // the time for the dependent loads of the replay) has the memory pipe free for -- instead of k_bk_sort storing a row of zeros per Gaussian
        // without a hit, piece by piece into five tensors (46 us of its 90 at S1M).  k_bwd_reduce4 runs two launches later and overwrites the rows
        // of the Gaussians with a hit; rows that span two of its waves are added onto these zeros with atomics as before.
        // zero_in_prep = 2: the SH gradients (192 of the 232 MB at M = 16) are left to k_bk_sort (one span per workgroup, rolling through the launch): cleared
        // here, up front, 232 MB of stores stood in the memory pipe before the first load of the replay (this launch lasted fill + replay: 50 + 95 us).
        bk_zero_span(p.d_means, 3 * P_, tid_, nthr_); bk_zero_span(p.d_scales, 2 * P_, tid_, nthr_); bk_zero_span(p.d_rots, 4 * P_, tid_, nthr_);
        bk_zero_span(p.d_opac, P_, tid_, nthr_);
        if (p.accum) bk_zero_span(p.accum, P_, tid_, nthr_);
        if (p.zero_in_prep != 2) bk_zero_span(p.d_shs, 3 * P_ * (size_t)p.M, tid_, nthr_);      // (an unaligned table: up front like the others)
    }
    if (MODE == 0) {
        __shared__ unsigned s_h16[16];
        bk_setup_cursors(p, s_cur, s_h16);
    }
    const unsigned gmask = (1u << p.bk_shift) - 1u;
    // A pair of rays costs two dependent round trips: the ray's hit count, then its upstream gradient, outputs and records.  The first one -- of the NEXT
    // pair -- is in flight while the current pair is replayed (round 6, last session; like the colour pass).
    const unsigned i2_step = 2u * (blockDim.x >> 6);
    unsigned r_nx = 0u; bool valid_nx = false; int n_nx = 0;
    { const unsigned i0 = 2u * (threadIdx.x >> 6);
      if (i0 < (unsigned)p.bk_rpg) { valid_nx = bk_group_ray(p, blockIdx.x, i0 + (unsigned)half, &r_nx); n_nx = valid_nx ? min(p.hit_n[r_nx], p.hit_cap) : 0; } }
    for (unsigned i2 = 2u * (threadIdx.x >> 6); i2 < (unsigned)p.bk_rpg; i2 += i2_step) {
        const unsigned r = r_nx;
        const bool valid = valid_nx;
        const int n = n_nx;
        valid_nx = false; n_nx = 0;
        if (i2 + i2_step < (unsigned)p.bk_rpg) { valid_nx = bk_group_ray(p, blockIdx.x, i2 + i2_step + (unsigned)half, &r_nx); n_nx = valid_nx ? min(p.hit_n[r_nx], p.hit_cap) : 0; }
        if (!__any(n > 0)) continue;
        const size_t rr = valid ? r : 0u;
        const float* dLp = p.dL_dout + LRT_NCH * rr; const float* fp = p.out9_in + LRT_NCH * rr;
        const float dL0 = dLp[0], dL1 = dLp[1], dL2 = dLp[2], dL3 = dLp[3], dL5 = dLp[5], dL6 = dLp[6], dL7 = dLp[7];
        const float f0 = fp[0], f1 = fp[1], f2 = fp[2], f3 = fp[3], f5 = fp[5], f6 = fp[6], f7 = fp[7], f8 = fp[8];
        if (MODE == 0 && hl < 4 && n > 0) {
            float4 v;
            if (hl == 0) v = make_float4(p.ray_o[3 * rr], p.ray_o[3 * rr + 1], p.ray_o[3 * rr + 2], dL3);
            else if (hl == 1) v = make_float4(p.ray_d[3 * rr], p.ray_d[3 * rr + 1], p.ray_d[3 * rr + 2], 0.f);
            else if (hl == 2) v = make_float4(dL0, dL1, dL2, 0.f);
            else v = make_float4(dL5, dL6, dL7, 0.f);
            p.ray_pk[4 * rr + hl] = v;
        }
        const float dL_dbg = dL0 * bg0 + dL1 * bg1 + dL2 * bg2;
        const bool need_n = (dL5 != 0.f) || (dL6 != 0.f) || (dL7 != 0.f);
        const bool any_n = __any(need_n && n > 0);
        float T_run = 1.f, rC0 = 0.f, rC1 = 0.f, rC2 = 0.f, rD = 0.f, rN0 = 0.f, rN1 = 0.f, rN2 = 0.f;
        float o[3], d[3], go[3] = {0.f, 0.f, 0.f}, gd[3] = {0.f, 0.f, 0.f}, db[16];     // MODE 1: the ray, this lane's share of its gradient
        if (MODE == 1) {
            for (int i = 0; i < 3; i++) { o[i] = p.ray_o[3 * rr + i]; d[i] = p.ray_d[3 * rr + i]; }
#pragma unroll
            for (int k = 0; k < 16; k++) db[k] = 0.f;
        }
        for (int cb = 0; __any(cb < n); cb += 32) {
            const int j = cb + hl;
            const bool live = j < n;
            const size_t id = rr * p.hit_cap + (live ? j : 0);
            const float t = p.hit_t[id];
            const int g = p.hit_g[id];
            const float4 cc = p.hit_pk[id];                          // written by k_fwd_colour
            const float c0 = cc.x, c1 = cc.y, c2 = cc.z; const bool cl0 = cc.w < 0.f;
            const float ao = fabsf(cc.w);                            // op * G, the clamp flag as its sign (k_fwd_colour)
            float n0 = 0.f, n1 = 0.f, n2 = 0.f;
            if (need_n && live) {                                    // normals only matter for upstream gradients on channels 5..7 (D3)
                const float q[4] = {p.rots[4 * (size_t)g], p.rots[4 * (size_t)g + 1], p.rots[4 * (size_t)g + 2], p.rots[4 * (size_t)g + 3]};
                float R[9];
                lrt_quat_to_R(q, R);
                n0 = R[2]; n1 = R[5]; n2 = R[8];
            }
            const float alpha = fminf(LRT_ALPHA_MAX, ao);
            const float incl = half_incl_prod(live ? (1.f - alpha) : 1.f);
            float excl = __shfl_up(incl, 1);
            if (hl == 0) excl = 1.f;
            const float Tk = T_run * excl;
            const float wgt = live ? alpha * Tk : 0.f;
            const float sC0 = rC0 + half_sum_f(wgt * c0), sC1 = rC1 + half_sum_f(wgt * c1), sC2 = rC2 + half_sum_f(wgt * c2);
            const float sD = rD + half_sum_f(wgt * t);
            float sN0 = rN0, sN1 = rN1, sN2 = rN2;
            if (any_n) { sN0 += half_sum_f(wgt * n0); sN1 += half_sum_f(wgt * n1); sN2 += half_sum_f(wgt * n2); }
            const float i1a = 1.0f / (1.0f - alpha);
            float dLa = dL0 * (Tk * c0 - (f0 - sC0) * i1a) + dL1 * (Tk * c1 - (f1 - sC1) * i1a) + dL2 * (Tk * c2 - (f2 - sC2) * i1a);
            dLa += dL_dbg * (-f8 * i1a);                             // D1 (backward.cu:595-598)
            dLa += dL3 * (Tk * t - (f3 - sD) * i1a);
            if (need_n) dLa += dL5 * (Tk * n0 - (f5 - sN0) * i1a) + dL6 * (Tk * n1 - (f6 - sN1) * i1a) + dL7 * (Tk * n2 - (f7 - sN2) * i1a);   // D3
            dLa *= (ao > LRT_ALPHA_MAX) ? 0.f : 1.f;                 // backward.cu:607-608
            if (MODE == 0 && live) {
                const unsigned slot = atomicAdd(&s_cur[(unsigned)g >> p.bk_shift], 1u);
                if (slot < p.rec_cap)
                    p.brec[slot] = make_uint4((r << p.bk_shift) | ((unsigned)g & gmask), __float_as_uint(t), __float_as_uint(dLa), __float_as_uint(cl0 ? -wgt : wgt));
            }
            if (MODE == 1 && live) {                                 // the hit's share of the ray gradient, as bwd_hit / k_bwd_reduce4 see the hit
                const float mu[3] = {p.means[3 * (size_t)g], p.means[3 * (size_t)g + 1], p.means[3 * (size_t)g + 2]};
                const float sc[2] = {p.scales[2 * (size_t)g], p.scales[2 * (size_t)g + 1]};
                const float q[4] = {p.rots[4 * (size_t)g], p.rots[4 * (size_t)g + 1], p.rots[4 * (size_t)g + 2], p.rots[4 * (size_t)g + 3]};
                LrtHitGeom hg;
                lrt_hit_geom(o, d, t, mu, sc, q, p.mod, &hg);
                lrt_hit_ray_backward(&hg, d, t, p.opac[g] * dLa, dL3 * wgt, go, gd);
                const float r0 = cl0 ? 0.f : dL0 * wgt, r1 = dL1 * wgt, r2 = dL2 * wgt;
                const float* sh = p.shs + (size_t)g * p.M * 3;
#pragma unroll
                for (int k = 0; k < 16; k++)
                    if (k < p.nsh) db[k] += r0 * sh[3 * k] + r1 * sh[3 * k + 1] + r2 * sh[3 * k + 2];
            }
            // carries for rays with more than 32 composited hits
            T_run *= half_last(incl, half);
            rC0 = half_last(sC0, half); rC1 = half_last(sC1, half); rC2 = half_last(sC2, half); rD = half_last(sD, half);
            if (any_n) { rN0 = half_last(sN0, half); rN1 = half_last(sN1, half); rN2 = half_last(sN2, half); }
        }
        if (MODE == 1) {                                             // colour term once per lane, then the half-wave's sums; lane 31 / 63 stores
            lrt_sh_basis_vjp(p.deg, d, db, gd);
            float s6[6];
            for (int i = 0; i < 3; i++) { s6[i] = half_sum_f(go[i]); s6[3 + i] = half_sum_f(gd[i]); }
            if (hl == 31 && valid && n > 0) store_ray_grad(p, r, s6, s6 + 3);
        }
    }
}

#ifdef LRT_LEGACY
// Sorted segmented reduction of the per-hit gradients (deterministic except for runs that span several waves): every lane of a wave takes
// ONE entry of the (g, id)-sorted hit list; the 58 per-hit components go through LDS as a [hit][component] matrix, lane c then
// walks its column hit by hit and adds; at the end of a run of equal gidx the 58 lanes store the Gaussian's gradient row with ONE
// store instruction (lane c -> component c).  No 58 x 6 dependent DPP steps and no 58 single-lane stores per run.
#define R3_STRIDE 59                       // odd row stride: conflict-free when lane = hit writes and when lane = component reads
__global__ void __launch_bounds__(256) k_bwd_reduce3(const TraceParams p)
{
    __shared__ float s_m[4][32 * R3_STRIDE];
    if (bwd_guard_skips(p)) return;
    const unsigned long long n_hits = p.n_hits_dev ? (unsigned long long)*p.n_hits_dev : (unsigned long long)p.n_hits;
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool live = i < n_hits;
    const unsigned long long wave0 = i - (unsigned long long)lane;
    const unsigned long long key = live ? p.sorted_keys[i] : ~0ull;
    const int g = live ? (int)(key >> p.id_bits) : -1;
    const unsigned id = (unsigned)(key & ((1ull << p.id_bits) - 1ull));
    const int nsh = p.nsh;
    float acc[10], ash[48];
#pragma unroll
    for (int k = 0; k < 10; k++) acc[k] = 0.f;
#pragma unroll
    for (int k = 0; k < 48; k++) ash[k] = 0.f;
    if (live) {
        const unsigned r = id / (unsigned)p.hit_cap;
        const float4 hp = p.hit_pk[id];
        const float4 r0_ = p.ray_pk[4 * (size_t)r], r1_ = p.ray_pk[4 * (size_t)r + 1], r2_ = p.ray_pk[4 * (size_t)r + 2], r3_ = p.ray_pk[4 * (size_t)r + 3];
        const float mu[3] = {p.means[3 * (size_t)g], p.means[3 * (size_t)g + 1], p.means[3 * (size_t)g + 2]};
        const float sc[2] = {p.scales[2 * (size_t)g], p.scales[2 * (size_t)g + 1]};
        const float q[4] = {p.rots[4 * (size_t)g], p.rots[4 * (size_t)g + 1], p.rots[4 * (size_t)g + 2], p.rots[4 * (size_t)g + 3]};
        const float op = p.opac[g];
        const float t = hp.x, da = hp.y, ws = hp.z, w = fabsf(ws);
        const float o[3] = {r0_.x, r0_.y, r0_.z}, d[3] = {r1_.x, r1_.y, r1_.z};
        LrtHitGeom hg;
        lrt_hit_geom(o, d, t, mu, sc, q, p.mod, &hg);
        const float dNgs[3] = {r3_.x * w, r3_.y * w, r3_.z * w};
        LrtHitGrad gr;
        lrt_hit_backward(&hg, o, d, mu, sc, q, op, op * da, r0_.w * w, dNgs, &gr);
        acc[0] = gr.d_mean[0]; acc[1] = gr.d_mean[1]; acc[2] = gr.d_mean[2];
        acc[3] = gr.d_scale[0]; acc[4] = gr.d_scale[1];
        acc[5] = gr.d_rot[0]; acc[6] = gr.d_rot[1]; acc[7] = gr.d_rot[2]; acc[8] = gr.d_rot[3];
        acc[9] = hg.G * da;
        float b[16];
        lrt_sh_basis(p.deg, d, b);
        const float c0 = (ws < 0.f) ? 0.f : r2_.x * w, c1 = r2_.y * w, c2 = r2_.z * w;
#pragma unroll
        for (int k = 0; k < 16; k++)
            if (k < nsh) { ash[3 * k] = b[k] * c0; ash[3 * k + 1] = b[k] * c1; ash[3 * k + 2] = b[k] * c2; }
    }
    const int wv = threadIdx.x >> 6;
    float* m = s_m[wv];
    const int gn = __shfl_down(g, 1);
    const bool tail = live && (lane == 63 || gn != g);
    const unsigned long long tails = __ballot(tail);
    if (!tails) return;
    // does the first / last run of this wave continue in a neighbouring wave?  (then its total is added atomically)
    const int g_first = __builtin_amdgcn_readlane(g, 0), g_last = __builtin_amdgcn_readlane(g, 63);
    bool sh_first = false, sh_last = false;
    if (wave0 > 0) sh_first = ((int)(p.sorted_keys[wave0 - 1] >> p.id_bits) == g_first);
    if (wave0 + 64 < n_hits) sh_last = ((int)(p.sorted_keys[wave0 + 64] >> p.id_bits) == g_last);
    const int nc = 10 + 3 * nsh;                               // live components
    const int M3 = p.M * 3;
    float run = 0.f;
    for (int half = 0; half < 2; half++) {
        if ((lane >> 5) == half) {                               // lanes of this half publish their hit's components
            float* row = m + (lane & 31) * R3_STRIDE;
#pragma unroll
            for (int k = 0; k < 10; k++) row[k] = acc[k];
#pragma unroll
            for (int k = 0; k < 48; k++) if (k < 3 * nsh) row[10 + k] = ash[k];
        }
        // wave-local LDS: in-order, no barrier needed inside a wave
        for (int j = 0; j < 32; j++) {
            const int hj = 32 * half + j;
            if (lane < nc) run += m[j * R3_STRIDE + lane];
            if ((tails >> hj) & 1ull) {
                const int gj = __builtin_amdgcn_readlane(g, hj);
                const bool shared = ((gj == g_first) && sh_first) || (hj == 63 && sh_last);
                if (lane < nc) {
                    float* dst = lane < 3 ? p.d_means + 3 * (size_t)gj + lane
                               : lane < 5 ? p.d_scales + 2 * (size_t)gj + (lane - 3)
                               : lane < 9 ? p.d_rots + 4 * (size_t)gj + (lane - 5)
                               : lane == 9 ? p.d_opac + gj
                               : p.d_shs + (size_t)gj * M3 + (lane - 10);
                    if (shared) unsafeAtomicAdd(dst, run); else *dst = run;
                }
                run = 0.f;
            }
        }
    }
}
#endif  // LRT_LEGACY
