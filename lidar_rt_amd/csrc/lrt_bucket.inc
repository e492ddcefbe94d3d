// lrt_bucket.inc -- the BUCKETED backward (bwd_mode 3; included by lrt_kernels.hip after lrt_backward.inc).
//
// The reference's backward re-traces every ray and adds every hit's 58 gradient components to the Gaussian with global atomics
// (DLT/optix_tracer/backward.cu:513-690).  The sorted backward of rounds 1-2 (bwd_mode 2) replays the forward's hit record, radix-sorts
// (Gaussian, hit) keys -- a histogram and three scatter passes over all hits -- and then GATHERS each hit's 16 bytes from its place
// in the ray-major record: one random sector per hit, the largest traffic item of the whole backward.  This path moves every hit
// exactly once instead:
//   k_bk_count   per GROUP of rays (<= 512 groups): hits per BUCKET of 2^s consecutive Gaussian indices (LDS histogram) -> M[group][bucket]
//   k_bk_scan    column-wise exclusive prefix of M over the groups (in 4 row blocks), hits per bucket and row block
//   k_bwd_prep<.,true>  the per-ray replay (lrt_backward.inc) writes each hit's 16-byte record to the next free slot of its bucket:
//                the cursors of a group are LDS words that start at base[bucket] + M[group][bucket] (base = exclusive prefix of the buckets'
//                totals, scanned by every workgroup for itself: bk_setup_cursors); no global atomics
//   k_bk_sort    one workgroup per bucket: counting sort of the bucket's records by Gaussian inside LDS -> one stream of records in
//                Gaussian order; rows of zeros for the Gaussians the reduction will not store whole
//   k_bwd_reduce4  the flat segmented reduction of k_bwd_reduce3 over that stream: no barriers, four workgroups per CU
// The order of the float additions inside a Gaussian's run is the arrival order of integer LDS atomics (cursor increments in
// k_bwd_prep and in the LDS sort) -- as in the reference's atomics, and as for runs that span waves in bwd_mode 2; everything else is
// deterministic.

#define BK_MAX_NB 16384                  // buckets (LDS cursors / histogram: 4 bytes each)
#define BK_MAX_NG 512                    // ray groups (rows of the count matrix)

// hits of a group of rays per bucket; one thread per ray
__global__ void __launch_bounds__(256) k_bk_count(const TraceParams p)
{
    extern __shared__ unsigned s_cnt[];
    if (bwd_guard_skips(p)) return;
    for (int b = threadIdx.x; b < p.bk_nb; b += 256) s_cnt[b] = 0u;
    __syncthreads();
    for (unsigned i = threadIdx.x; i < (unsigned)p.bk_rpg; i += 256) {
        unsigned r;
        if (!bk_group_ray(p, blockIdx.x, i, &r)) continue;
        const int n = min(p.hit_n[r], p.hit_cap);
        const int* gp = p.hit_g + (size_t)r * p.hit_cap;
        // eight entries per trip, loaded before the first LDS atomic: one load -> atomic round trip per ENTRY made the ~30 entries of a ray a
        // chain of 30 dependent steps (14 us for the launch)
        int j = 0;
        for (; j + 8 <= n; j += 8) {
            int g[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) g[u] = gp[j + u];
#pragma unroll
            for (int u = 0; u < 8; ++u) atomicAdd(&s_cnt[(unsigned)g[u] >> p.bk_shift], 1u);
        }
        {
            int g[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) g[u] = (j + u < n) ? gp[j + u] : -1;
#pragma unroll
            for (int u = 0; u < 8; ++u) if (g[u] >= 0) atomicAdd(&s_cnt[(unsigned)g[u] >> p.bk_shift], 1u);
        }
    }
    __syncthreads();
    unsigned* row = p.bk_M + (size_t)blockIdx.x * p.bk_nb;
    for (int b = threadIdx.x; b < p.bk_nb; b += 256) row[b] = s_cnt[b];
}

// Column-wise exclusive prefix of M over the ray groups, in BK_RB row blocks so that the launch fills the chip: workgroup (x, y) takes
// 64 buckets and the groups [y * rbg, (y + 1) * rbg); M[w][b] <- sum of M[w'][b] over the groups w' < w of the SAME row block, and the
// block's column totals go to aux[y][b] (k_bwd_prep adds the totals of the earlier row blocks when it sets up its cursors).
// Thread = (bucket, one of 16 chunks of the block's groups).
__global__ void __launch_bounds__(1024) k_bk_scan(const TraceParams p)
{
    __shared__ unsigned s_part[16][64];
    if (bwd_guard_skips(p)) return;
    const int bl = threadIdx.x & 63, c = threadIdx.x >> 6;
    const int b = blockIdx.x * 64 + bl;
    const int rbg = (p.bk_ng + BK_RB - 1) / BK_RB;
    const int g0 = blockIdx.y * rbg, g1 = min(g0 + rbg, p.bk_ng);
    const int ch = (rbg + 15) / 16;
    const int w0 = min(g0 + c * ch, g1), w1 = min(w0 + ch, g1);
    unsigned sum = 0u;
    if (b < p.bk_nb) for (int w = w0; w < w1; ++w) sum += p.bk_M[(size_t)w * p.bk_nb + b];
    s_part[c][bl] = sum;
    __syncthreads();
    unsigned run = 0u, tot = 0u;
    for (int k = 0; k < 16; ++k) { const unsigned v = s_part[k][bl]; if (k < c) run += v; tot += v; }
    if (b >= p.bk_nb) return;
    for (int w = w0; w < w1; ++w) { unsigned* q = p.bk_M + (size_t)w * p.bk_nb + b; const unsigned v = *q; *q = run; run += v; }
    if (c == 0) p.bk_aux[(size_t)blockIdx.y * p.bk_nb + b] = tot;
}

// One Gaussian's gradient row, lane = component: lanes 0..2 mean, 3..4 scale, 5..8 rotation, 9 opacity, 10.. SH (row width M3).
// add = false: plain stores (the caller owns the row); true: float atomics on a row that starts from zero.
// The lane's column of the row is fixed for the whole launch: its tensor, the offset inside that tensor's row and the row stride are formed ONCE
// (bk_row_lane), a row then costs one 64-bit multiply-add and the store (the five-way pointer select per row was ~30 instructions).
struct BkRowLane { float* base; unsigned stride; };
__device__ __forceinline__ BkRowLane bk_row_lane(const TraceParams& p, int lane, int nrow, int M3)
{
    BkRowLane r;
    r.base = lane < 3 ? p.d_means + lane : lane < 5 ? p.d_scales + (lane - 3) : lane < 9 ? p.d_rots + (lane - 5) : lane == 9 ? p.d_opac : p.d_shs + (lane - 10);
    r.stride = lane < 3 ? 3u : lane < 5 ? 2u : lane < 9 ? 4u : lane == 9 ? 1u : (unsigned)M3;
    if (lane >= nrow) r.base = nullptr;
    if (lane == nrow && p.accum) { r.base = p.accum; r.stride = 1u; }      // option deferred_accum: the lane behind the row carries the Gaussian's sum of composite weights (the launcher keeps nrow < 64)
    return r;
}
__device__ __forceinline__ void bk_row_out(const BkRowLane& rl, size_t gj, float v, bool add)
{
    if (!rl.base) return;
    float* dst = rl.base + gj * rl.stride;
    if (add) unsafeAtomicAdd(dst, v); else *dst = v;
}

// One workgroup per bucket: counting sort of the bucket's records by Gaussian (integer LDS atomics: histogram, scan by one wave,
// cursors) -> the stream of all records in Gaussian order, brec2 (ray, t, dL/dalpha, +-w) and bg (Gaussian).  The bucket was just
// written and is read twice: the second read and the scattered 16-byte writes stay inside a few KB that the caches hold.
// The same workgroup prepares the gradient rows the reduction will not store whole: zeros for Gaussians without a hit, and zeros for
// the Gaussians whose run of records crosses a border between two waves of k_bwd_reduce4 (positions 64 w), whose pieces are added
// with atomics -- so the 232 MB memset of the gradient tensors is gone.
#ifndef BK_DET_LONG
#define BK_DET_LONG 96u                  // option deterministic: runs longer than this are ordered through the ray bitmap
#endif
__global__ void __launch_bounds__(256) k_bk_sort(const TraceParams p)
{
    extern __shared__ unsigned s_u[];
    const int Gb = 1 << p.bk_shift;
    unsigned* s_off = s_u;               // [Gb + 1] first sorted position of a Gaussian's records
    unsigned* s_cnt = s_u + Gb + 1;      // [Gb] histogram, then cursors
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int b = (int)blockIdx.x;
    if (bwd_guard_skips(p)) { if (!p.prezeroed) bk_zero_rows(p, b, tid, 256); return; }   // the re-tracing fallback behind this launch adds with atomics
    if (p.zero_in_prep == 2) {           // this workgroup's span of the SH gradient table <- 0 (16-byte aligned whole float4s: the launcher checked); see k_bwd_prep2
        const unsigned long long n4 = ((unsigned long long)p.P * (unsigned long long)p.M * 3ull) >> 2;
        const unsigned long long z0 = n4 * (unsigned)b / gridDim.x, z1 = n4 * ((unsigned)b + 1u) / gridDim.x;
        float4* const z4 = reinterpret_cast<float4*>(p.d_shs);
        for (unsigned long long i = z0 + (unsigned)tid; i < z1; i += 256ull) z4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const unsigned lo = min(p.bk_base[b], p.rec_cap), hi = min(p.bk_base[b + 1], p.rec_cap);
    const int n = (int)(hi - lo);
    const unsigned gmask = (unsigned)(Gb - 1);
    const uint4* rec = p.brec + lo;
    for (int i = tid; i < Gb; i += 256) s_cnt[i] = 0u;
    __syncthreads();
    for (int i = tid; i < n; i += 256) atomicAdd(&s_cnt[rec[i].x & gmask], 1u);
    __syncthreads();
    if (wv == 0) {                       // exclusive scan of up to 512 counts by one wave: 8 (or fewer) consecutive counts per lane
        const int per = (Gb + 63) >> 6;
        unsigned c[8], sum = 0u;
#pragma unroll
        for (int k = 0; k < 8; k++) { c[k] = (k < per && lane * per + k < Gb) ? s_cnt[lane * per + k] : 0u; sum += c[k]; }
        unsigned incl = sum;
        for (int o = 1; o < 64; o <<= 1) { const unsigned v = __shfl_up(incl, o); if (lane >= o) incl += v; }
        unsigned run = incl - sum;
#pragma unroll
        for (int k = 0; k < 8; k++) if (k < per && lane * per + k < Gb) { s_off[lane * per + k] = run; s_cnt[lane * per + k] = run; run += c[k]; }
        if (lane == 63) s_off[Gb] = incl;
    }
    __syncthreads();
    const unsigned g0 = (unsigned)b << p.bk_shift;
    for (int i = tid; i < n; i += 256) {
        const uint4 rc = rec[i];
        const unsigned gl = rc.x & gmask;
        const unsigned pos = lo + atomicAdd(&s_cnt[gl], 1u);
        p.brec2[pos] = make_uint4(rc.x >> p.bk_shift, rc.y, rc.z, rc.w);
        p.bkg[pos] = g0 + gl;
    }
    if (p.deterministic) {
        // The cursors above hand out a run's places in the arrival order of LDS atomics, and the reduction adds a run up in the order it finds it.
        // Second pass: every record to the place of its RAY inside its Gaussian's run (a Gaussian is hit once per ray: the ranks are a permutation) --
        // from brec2 back into this bucket's span of brec, which the first pass has consumed; k_bwd_reduce4 then reads brec.
        //   * a run of <= BK_DET_LONG records: a thread per record counts the smaller rays of its run (cached: the workgroup just wrote them);
        //   * a longer run (a large Gaussian close to the sensor is hit by thousands of rays: the counting loop is quadratic, 8.7 ms per S1M frame
        //     when it did all runs): the workgroup marks the run's rays in a bitmap over the image, counts the marks word by word (a prefix
        //     per thread's chunk of words) and a record's place is the number of marks below its ray.
        __syncthreads();
        const unsigned words = (unsigned)p.det_bm_words;              // 0: the image does not fit the bitmap -- every run takes the counting loop
        bool any_long = false;
        for (int i = tid; i < n; i += 256) {
            const unsigned pos = lo + (unsigned)i;
            const unsigned ray = p.brec2[pos].x;
            const unsigned gl = p.bkg[pos] - g0;
            const unsigned a = lo + s_off[gl], e = lo + s_off[gl + 1];
            if (words && e - a > BK_DET_LONG) { any_long = true; continue; }
            unsigned k = 0u;
            for (unsigned j = a; j < e; j++) k += (p.brec2[j].x < ray) ? 1u : 0u;
            p.brec[a + k] = p.brec2[pos];
        }
        if (__syncthreads_or(any_long ? 1 : 0)) {
            unsigned* const bm = s_u + 2 * Gb + 1;                   // [words] one bit per ray
            unsigned* const s_cs = bm + words;                       // [256] marks in front of a thread's chunk of words
            const unsigned chunk = (words + 255u) >> 8;
            for (unsigned k = (unsigned)tid; k < words; k += 256u) bm[k] = 0u;
            for (int gl = 0; gl < Gb; gl++) {
                const unsigned a = lo + s_off[gl], e = lo + s_off[gl + 1];
                if (e - a <= BK_DET_LONG) continue;                  // (uniform)
                __syncthreads();                                     // the bitmap is clear
                for (unsigned j = a + (unsigned)tid; j < e; j += 256u) { const unsigned r = p.brec2[j].x; atomicOr(&bm[r >> 5], 1u << (r & 31u)); }
                __syncthreads();
                { unsigned c = 0u; const unsigned k0 = (unsigned)tid * chunk, k1 = min(k0 + chunk, words);
                  for (unsigned k = k0; k < k1; k++) c += (unsigned)__popc(bm[k]);
                  s_cs[tid] = c; }
                __syncthreads();
                if (wv == 0) {                                       // exclusive scan of the 256 chunk counts by one wave
                    unsigned c4[4], sum = 0u;
#pragma unroll
                    for (int k = 0; k < 4; k++) { c4[k] = s_cs[4 * lane + k]; sum += c4[k]; }
                    unsigned incl = sum;
                    for (int o = 1; o < 64; o <<= 1) { const unsigned v = __shfl_up(incl, o); if (lane >= o) incl += v; }
                    unsigned run = incl - sum;
#pragma unroll
                    for (int k = 0; k < 4; k++) { s_cs[4 * lane + k] = run; run += c4[k]; }
                }
                __syncthreads();
                for (unsigned j = a + (unsigned)tid; j < e; j += 256u) {
                    const unsigned ray = p.brec2[j].x;
                    const unsigned w_ = ray >> 5, t_ = w_ / chunk;
                    unsigned k = s_cs[t_] + (unsigned)__popc(bm[w_] & ((1u << (ray & 31u)) - 1u));
                    for (unsigned q = t_ * chunk; q < w_; q++) k += (unsigned)__popc(bm[q]);
                    p.brec[a + k] = p.brec2[j];
                }
                __syncthreads();
                for (unsigned j = a + (unsigned)tid; j < e; j += 256u) bm[p.brec2[j].x >> 5] = 0u;      // (only the words this run touched)
            }
        }
    }
    if (p.prezeroed || p.zero_in_prep) return;             // the caller keeps the tensors all-zero between steps / k_bwd_prep2 cleared them whole: nothing to clear
    const int M3 = 3 * p.M, nrow = 10 + M3;
    // (option deferred_accum: the lane behind the row clears the weight too -- the tensor the caller hands over may hold anything, e.g. the
    // sharded tracer's reused exchange buffer; the default, zero_in_prep, never gets here)
    const BkRowLane rl = bk_row_lane(p, lane, nrow, M3);
    for (int gb = wv * 64; gb < Gb; gb += 256) {
        const int gq = gb + lane;
        bool z = false, cross = false;
        if (gq < Gb && (size_t)g0 + gq < (size_t)p.P) {
            const unsigned a = lo + s_off[gq], e = lo + s_off[gq + 1];
            cross = (a != e) && ((a >> 6) != ((e - 1u) >> 6));
            z = (a == e) || cross;
        }
        for (unsigned long long rest = __ballot(z); rest; rest &= rest - 1ull) {
            const int j = __builtin_ctzll(rest);
            bk_row_out(rl, (size_t)g0 + gb + j, 0.f, false);
        }
    }
}

// The reduction over the sorted stream: every lane of a wave takes ONE record (positions 64 w .. 64 w + 63), evaluates the hit's
// gradient; the 10 + 3*nsh components go through LDS as a [record][component] matrix, lane = component adds down its column and the
// Gaussian's row goes out at the end of its run: stored whole when the run lies inside the wave, added with atomics (onto the zeros
// k_bk_sort left) when it continues in a neighbouring wave.  The arithmetic is k_bwd_reduce3's; the record arrives in sequence
// instead of through a sorted key and a 16-byte gather.
#define R4_STRIDE 60                     // 16-byte rows (ds_write_b128); 32 lanes x 240 B cover all banks twice
#ifndef R4_PASS
#define R4_PASS 16                       // records of a wave staged per pass (a multiple of 8, divides 64): 16 -> 15 KB of LDS per workgroup
#endif
#ifndef R4_OCC
#define R4_OCC 7                         // workgroups per CU = waves per SIMD: 72 registers (the build runs without the SLP vectoriser: 69; with it 94)
#endif
// time = 67 us + 360 us / workgroups per CU (round-4 fit): 5 workgroups (96 registers, 32 records per pass = 30 KB of LDS) 138 us
__global__ void __launch_bounds__(256, R4_OCC) k_bwd_reduce4(const TraceParams p)
{
    __shared__ __attribute__((aligned(16))) float s_m[4][R4_PASS * R4_STRIDE];
    if (bwd_guard_skips(p)) return;
    const unsigned n_hits = min(p.bk_base[p.bk_nb], p.rec_cap);
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const unsigned wave0 = i - (unsigned)lane;
    if (wave0 >= n_hits) return;
    const bool live = i < n_hits;
    const int g = live ? (int)p.bkg[i] : -1;
    const int nsh = p.nsh;
    // the 48 SH components of a record are products basis[k] x colour[ch]: kept as 16 + 3 factors and multiplied when the row is written
    // (with the closed-form geometry chain the 58 finished components were the kernel's register peak)
    float acc[10], bs[16], cc[3] = {0.f, 0.f, 0.f}, wacc = 0.f;
#pragma unroll
    for (int k = 0; k < 10; k++) acc[k] = 0.f;
#pragma unroll
    for (int k = 0; k < 16; k++) bs[k] = 0.f;
    if (live) {
        const uint4 rc = p.brec2[i];
        const unsigned r = rc.x;
        const float t = __uint_as_float(rc.y), da = __uint_as_float(rc.z), ws = __uint_as_float(rc.w), w = fabsf(ws);
        const float4 r0_ = p.ray_pk[4 * (size_t)r], r1_ = p.ray_pk[4 * (size_t)r + 1], r2_ = p.ray_pk[4 * (size_t)r + 2], r3_ = p.ray_pk[4 * (size_t)r + 3];
        const float mu[3] = {p.means[3 * (size_t)g], p.means[3 * (size_t)g + 1], p.means[3 * (size_t)g + 2]};
        const float sc[2] = {p.scales[2 * (size_t)g], p.scales[2 * (size_t)g + 1]};
        const float q[4] = {p.rots[4 * (size_t)g], p.rots[4 * (size_t)g + 1], p.rots[4 * (size_t)g + 2], p.rots[4 * (size_t)g + 3]};
        const float op = p.opac[g];
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
        lrt_sh_basis(p.deg, d, bs);
#pragma unroll
        for (int k = 0; k < 16; k++) bs[k] = (k < nsh) ? bs[k] : 0.f;
        cc[0] = (ws < 0.f) ? 0.f : r2_.x * w; cc[1] = r2_.y * w; cc[2] = r2_.z * w;
        wacc = w;
    }
    float* m = s_m[threadIdx.x >> 6];
    const int gn = __shfl_down(g, 1);
    const bool tail = live && (lane == 63 || gn != g);
    const unsigned long long tails = __ballot(tail);
    // does the first / last run of this wave continue in a neighbouring wave?  (then its total is added atomically)
    const int g_first = __builtin_amdgcn_readlane(g, 0), g_last = __builtin_amdgcn_readlane(g, 63);
    bool sh_first = false, sh_last = false;
    if (wave0 > 0u) sh_first = ((int)p.bkg[wave0 - 1u] == g_first);
    if (wave0 + 64u < n_hits) sh_last = ((int)p.bkg[wave0 + 64u] == g_last);
    const int nc = 10 + 3 * nsh, M3 = p.M * 3, nrow = 10 + M3;
    const BkRowLane rl = bk_row_lane(p, lane, nrow, M3);
    // option deferred_accum: column 58 of the staged matrix (free: nc <= 58) holds the hit's composite weight, lane `nrow` adds it up like a
    // gradient component and stores forward.cu:268's per-Gaussian sum -- the forward then needs no float atomic per composited hit
    const bool col_on = (lane < nc) || (p.accum != nullptr && lane == nrow);
    const int col = lane < nc ? lane : 58;
    float run = 0.f;
#pragma unroll 1
    for (int half = 0; half < 64 / R4_PASS; half++) {
        // (opaque per pass: the 48 SH products below are loop invariant, and hoisted out of the loop they are 48 live registers)
        asm volatile("" : "+v"(cc[0]), "+v"(cc[1]), "+v"(cc[2]));
        if ((lane / R4_PASS) == half) {                          // lanes of this part of the wave publish their record's components: 15 x 16 bytes
            float4* row = (float4*)(m + (lane % R4_PASS) * R4_STRIDE);
#define R4_ASH(j_) (bs[(j_) / 3] * cc[(j_) % 3])
            row[0] = make_float4(acc[0], acc[1], acc[2], acc[3]); row[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
            row[2] = make_float4(acc[8], acc[9], R4_ASH(0), R4_ASH(1));
#pragma unroll
            for (int k = 0; k < 11; k++) row[3 + k] = make_float4(R4_ASH(2 + 4 * k), R4_ASH(3 + 4 * k), R4_ASH(4 + 4 * k), R4_ASH(5 + 4 * k));
            row[14] = make_float4(R4_ASH(46), R4_ASH(47), wacc, 0.f);
#undef R4_ASH
        }
        // wave-local LDS: in-order, no barrier needed inside a wave.  Lane = component reads 8 values of its column at once (one LDS
        // latency instead of eight), forms the running sums -- restarting behind every end of a run -- and writes them back in
        // place; the ends of runs then pick their sums up.
        for (int qr = 0; qr < R4_PASS / 8; qr++) {
            const unsigned e16 = (unsigned)(tails >> (R4_PASS * half + 8 * qr)) & 0xffu;
            float* mq = m + qr * 8 * R4_STRIDE;
            if (col_on) {
                float mv[8];
#pragma unroll
                for (int j = 0; j < 8; j++) mv[j] = mq[j * R4_STRIDE + col];
                if (e16 == 0u) {                                   // (uniform) no run ends among these eight records -- three blocks in four: a Gaussian's
                                                                   // run is 34 records long on average -- nobody reads the partial sums back
#pragma unroll
                    for (int j = 0; j < 8; j++) run += mv[j];      // (the same additions in the same order)
                } else {
#pragma unroll
                    for (int j = 0; j < 8; j++) { run += mv[j]; mv[j] = run; run = ((e16 >> j) & 1u) ? 0.f : run; }
#pragma unroll
                    for (int j = 0; j < 8; j++) mq[j * R4_STRIDE + col] = mv[j];
                }
            }
            for (unsigned rest = e16; rest; rest &= rest - 1u) {
                const int j = __builtin_ctz(rest), hj = R4_PASS * half + 8 * qr + j;
                const int gj = __builtin_amdgcn_readlane(g, hj);
                const bool shared = ((gj == g_first) && sh_first) || (hj == 63 && sh_last);
                const float v_ = col_on ? mq[j * R4_STRIDE + col] : 0.f;
                if (shared && p.det_part)      // option deterministic: the piece goes to this wave's row F (the run began in an earlier wave) or L (it goes on in the next); k_bwd_fixup adds the pieces in wave order
                    p.det_part[(2 * (size_t)(wave0 >> 6) + (((gj == g_first) && sh_first) ? 0u : 1u)) * 64 + (unsigned)lane] = v_;
                else bk_row_out(rl, (size_t)gj, v_, shared);
            }
        }
    }
}

// Option deterministic: the total of a run of records that crosses waves of k_bwd_reduce4.  Wave w of the reduction left L(w), the piece of its
// last run when that run goes on in wave w + 1, and F(w), the piece of its first run when that run began before w (a wave that lies inside one
// run has F only).  The wave where a run begins adds L(w) + F(w + 1) + F(w + 2) ... in this order and stores the row whole -- float atomics
// would add three or more pieces in the order of their arrival.  One wave of this launch per wave of the reduction; lane = component.
__global__ void __launch_bounds__(256) k_bwd_fixup(const TraceParams p)
{
    if (bwd_guard_skips(p)) return;
    const unsigned n_hits = min(p.bk_base[p.bk_nb], p.rec_cap);
    const unsigned w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    const unsigned wave0 = w << 6;
    if (wave0 + 64u >= n_hits) return;                               // no wave behind this one
    const unsigned g_last = p.bkg[wave0 + 63u];
    if (p.bkg[wave0 + 64u] != g_last) return;                        // the last run ends with the wave
    const unsigned g_first = p.bkg[wave0];
    if (g_first == g_last && wave0 > 0u && p.bkg[wave0 - 1u] == g_first) return;      // the run began earlier: its first wave adds it up
    const int nc = 10 + 3 * p.nsh, M3 = p.M * 3, nrow = 10 + M3;
    const BkRowLane rl = bk_row_lane(p, lane, nrow, M3);
    const bool col_on = (lane < nc) || (p.accum != nullptr && lane == nrow);
    float sum = p.det_part[(2 * (size_t)w + 1) * 64 + (unsigned)lane];
    for (unsigned w2 = w + 1u; ; w2++) {
        sum += p.det_part[(2 * (size_t)w2) * 64 + (unsigned)lane];
        const unsigned b2 = w2 << 6;
        if (!(b2 + 64u < n_hits && p.bkg[b2 + 63u] == g_last && p.bkg[b2 + 64u] == g_last)) break;      // wave w2 holds the run's end
    }
    bk_row_out(rl, (size_t)g_last, col_on ? sum : 0.f, false);
}
