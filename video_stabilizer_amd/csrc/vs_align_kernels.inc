// vs_align_kernels.inc -- the per-pair device code of the aligner (Gauss-Newton level, on-device introselect, the fused
// all-levels kernel).  Included by vs_engine.hip once per workgroup size, inside a namespace that defines kGnThreads.
// ---- Gauss-Newton level solver: alignment.cpp:548-688 -------------------------------------------
// Runs inside a workgroup that owns one frame pair.  H = sum j j^T (fp64) -> cond / Tikhonov /
// pseudo-inverse once, then up to max_iters iterations of { sparse_ica (generators.cpp:429-596) ->
// dt = Hinv b -> delta.compose(T) -> corner test }, all without leaving the device.  Every thread
// carries the (identical) fp64 transform in registers; the only exchange per iteration is the block
// sum.  T is updated in place (including the x2 of TX,TY when moving to a finer level).
// Returns 0 ok / 2 max iterations / 3 over displacement; *iters_out, *cond_out as the reference logs.
#define VS_LDS_AS __attribute__((address_space(3)))
// Virtual threads.  Every fp64 sum of a pair is defined over kGnVirt threads (which records a thread adds, in which order, and
// the fixed trees that combine lanes and waves).  A build whose workgroup has fewer hardware threads (kGnThreads < kGnVirt: the
// small-footprint batch kernel, 256 threads standing in for 512) walks the virtual threads / waves it stands in for one after the
// other, each with its own accumulators, and parks the per-virtual-wave partial sums exactly where the full-size build does:
// the same additions on the same operands in the same order, so the results are bit-identical across the builds.
constexpr int kVF = kGnVirt / kGnThreads;        // virtual threads per hardware thread (1 or 2)
constexpr int kVWaves = kGnVirt / 64;            // virtual waves
constexpr int kRWaves = kGnThreads / 64;         // hardware waves
static_assert(kGnVirt % kGnThreads == 0 && (kVF == 1 || (kVF == 2 && kRWaves == 4)), "virtual-thread layouts: 1:1, or 256 threads for 512");
struct GnShared {
    double red[2][kVWaves * 10];
    double hinv[17];
    double c0[8];   // corners at level start
    double c1[8];   // corners after the previous iteration (only wave 0 needs them: kept out of everybody's registers)
    double T[4];    // the transform after the current iteration, published by wave 0
    int flag;       // 0 iterate on / 1 converged / 2 out of iterations / 3 over max_displacement
    // pipelined loop (coarsest level).  Wave 0 runs up to one barrier ahead of the slowest reader, so what it publishes
    // is double-buffered by iteration parity.
    double Tp[2][4];   // Tp[k & 1] = the transform after iteration k
    int seq;           // number of transforms published so far (k + 1 once Tp[k & 1] is valid)
    int ctl[2];        // ctl[k & 1] = (k + 1) << 2 | flag, written once wave 0 has done the convergence test of iteration k
};

// Hessian of a level (alignment.cpp:278-332): per-wave partial sums of the upper triangle of sum j j^T over both sets, in
// fp64, parked in sh.red[0] -- and the sums of the level's FIRST Gauss-Newton pass (generators.cpp:429-596 with the residuals the
// records already hold, PointRecs::r0), parked in sh.red[1] (every wave's eight sums, wave 0 included).  Thread t adds
// records t, t + kGnThreads, ... in that order.  The caller puts a barrier behind it.  The fused kernel accumulates the same
// sums, in the same order, while it writes the records (vs_k_align_pairs) and does not call this.
// (the set is chosen by zeroing the residual, not by a branch over the two halves of a8: the compiler folds such a branch into
// a select of the array index, and a private array indexed by a register lives in scratch memory.  Adding the +-0 products
// of the other set's records changes no sum.)
__device__ __forceinline__ void first_pass_terms(int r, int nsel, const float jf[4], float residual, double (&a8)[8]) {
    const float rx = r < nsel ? residual : 0.0f, ry = r < nsel ? 0.0f : residual;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        a8[c] += (double)(jf[c] * rx);
        a8[4 + c] += (double)(jf[c] * ry);
    }
}
__device__ __noinline__ void gn_hessian_partials(GnShared& sh, const PointRecs& rc, int nsel) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    const VS_GLOBAL_AS f32x4* __restrict__ rj = (const VS_GLOBAL_AS f32x4*)uniform_ptr(rc.j);
    const VS_GLOBAL_AS float* __restrict__ rr0 = (const VS_GLOBAL_AS float*)uniform_ptr(rc.r0);
    nsel = __builtin_amdgcn_readfirstlane(nsel);
    for (int v = 0; v < kVF; v++) {                     // virtual thread threadIdx.x + v * kGnThreads (virtual wave: + v * kRWaves)
        double hacc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        double a8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int r = threadIdx.x + v * kGnThreads; r < 2 * nsel; r += kGnVirt) {
            const f32x4 jf = rj[r];
            const float r0 = rr0[r];
            const double j[4] = {(double)jf.x, (double)jf.y, (double)jf.z, (double)jf.w};
            int k = 0;
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
                for (int b = a; b < 4; b++) hacc[k++] += j[a] * j[b];
            const float jv[4] = {jf.x, jf.y, jf.z, jf.w};
            first_pass_terms(r, nsel, jv, r0, a8);
        }
        const int vwave = ((int)threadIdx.x >> 6) + v * kRWaves;
        wave_partials_at<10>(hacc, sh.red[0], vwave);
        wave_partials8_butterfly(a8, sh.red[1], vwave);
    }
}

// key_lds: the same level image staged in LDS (padded by 8 bytes), or nullptr -- then the samples gather from global memory.
// On entry sh.red[0] holds the Hessian partials (gn_hessian_partials or the fused kernel's gather) and a barrier has passed.
__device__ __noinline__ int gn_level(GnShared& sh_g, const uint8_t* __restrict__ key, const uint8_t* key_lds, int w, int h, int nsel,
                                        const PointRecs& rc, int level, const GnParams& gp_in, double T_io[4], int* iters_out,
                                        double* cond_out) {
    // This function is not inlined, so its arguments arrive as per-lane values and generic pointers.  They are the same
    // in every lane and all point to device memory: say so (readfirstlane -> SGPRs; address space 1 -> global_load with a
    // scalar base instead of flat_load with a 64-bit address per lane; address space 3 for the shared block).  The
    // transform and the parameters are copied into registers once: behind their pointers (the caller's stack) every use
    // inside the loop would be a flat access to scratch memory.
    VS_LDS_AS GnShared& sh = *(VS_LDS_AS GnShared*)(uintptr_t)__builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)&sh_g);
    const vs_gbytes gkey = (vs_gbytes)uniform_ptr(key);
    const vs_lbytes lkey = (vs_lbytes)(uintptr_t)__builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)key_lds);   // LDS offset (low 32 bits), 0 = none
    const bool from_lds = __builtin_amdgcn_readfirstlane(key_lds != nullptr ? 1 : 0) != 0;
    w = __builtin_amdgcn_readfirstlane(w); h = __builtin_amdgcn_readfirstlane(h);
    nsel = __builtin_amdgcn_readfirstlane(nsel); level = __builtin_amdgcn_readfirstlane(level);
    const int max_iters = __builtin_amdgcn_readfirstlane(gp_in.max_iters);
    const double threshold = gp_in.threshold, max_displacement = gp_in.max_displacement;
    double T[4] = {T_io[0], T_io[1], T_io[2], T_io[3]};
    const VS_GLOBAL_AS uint32_t* __restrict__ rxy = (const VS_GLOBAL_AS uint32_t*)uniform_ptr(rc.xy);
    const VS_GLOBAL_AS float* __restrict__ rtv = (const VS_GLOBAL_AS float*)uniform_ptr(rc.tv);
    typedef float f32x4 __attribute__((ext_vector_type(4)));     // float4 records, read as a plain vector (HIP's float4 is a class)
    const VS_GLOBAL_AS f32x4* __restrict__ rj = (const VS_GLOBAL_AS f32x4*)uniform_ptr(rc.j);
    // Work split inside the workgroup: wave 0 does the scalar work of the level (Hessian sum, eigen-solve, the transform
    // update and the corner test: dependent fp64 chains), waves 1.. do the sampling of sparse_ica (generators.cpp:429-596).
    // The points of both sets (records are stored x-set first, then y-set) are dealt to the sampler waves in chunks of 64,
    // round robin.  With 512 threads, wave 4 shares its SIMD with wave 0 only (a workgroup's waves go to the SIMDs round
    // robin): a wave that runs alone reaches ~3/4 of the throughput of a pair, so on small levels it gets one chunk in
    // five and the other six waves share the rest (measured per chunk: ~1400 cycles alone, ~1090 per pair).  The rule depends
    // on the thread count and the number of points only, so the fused kernel and the per-level kernel add the same partial
    // sums in the same order.
    // (the waves of this rule are VIRTUAL waves: a 256-thread build has hardware wave 0 do the scalar work and hardware waves
    // 1..3 walk virtual waves {1,4}, {2,5,7}, {3,6} one after the other -- 1/3, 2/5 and 4/15 of the points under the weighted rule)
    constexpr int kWaves = kVWaves, kRecChunks = 8;
    const bool w0 = threadIdx.x < 64;
    const int rwave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    int wave = rwave;                                                   // the virtual wave this hardware wave is standing in for
    const int end = 2 * nsel, nchunk = (end + 63) >> 6;
    const bool weighted = kWaves == 8 && nchunk <= 5 * kRecChunks;
    // chunk number `slot` of virtual wave `wave` (slots are visited in increasing order; a slot past the end gives a chunk >= nchunk)
    auto chunk_of = [&](int slot) -> int {
        if (!weighted) return wave - 1 + slot * (kWaves - 1);
        if (wave == 4) return 5 * slot + 4;
        const int w_other = wave < 4 ? wave - 1 : wave - 2;          // this wave's place among the six waves other than 0 and 4
        const int idx = w_other + 6 * slot;                            // its idx-th chunk among those that are not wave 4's
        return (idx >> 2) * 5 + (idx & 3);
    };
    // the virtual waves of hardware sampler wave rwave >= 1: n-th of them, or -1
    auto vwave_of = [&](int n) -> int {
        if (kVF == 1) return n == 0 ? rwave : -1;
        return n < 2 ? rwave + 3 * n : ((n == 2 && rwave == 2) ? 7 : -1);      // {1,4}, {2,5,7}, {3,6}
    };
    // accumulators: a8[0..3] the x-set, a8[4..7] the y-set.  Two separate conditions on purpose: an if / else over the two
    // halves of one array is folded into a select of the array index, and a private array indexed by a register lives in
    // scratch memory.
    auto residual_terms = [&](int r, const f32x4& jf, float residual, double (&a8)[8]) {
        const double p0 = (double)(jf.x * residual), p1 = (double)(jf.y * residual), p2 = (double)(jf.z * residual),
                     p3 = (double)(jf.w * residual);
        const bool in_x = r < nsel, in_y = r >= nsel && r < end;
        if (in_x) { a8[0] += p0; a8[1] += p1; a8[2] += p2; a8[3] += p3; }
        if (in_y) { a8[4] += p0; a8[5] += p1; a8[6] += p2; a8[7] += p3; }
    };
    // One sampling pass with the records read from memory, two chunks in flight per wave: all their record loads and row
    // gathers are issued before the first is consumed, and the next pair's coordinates (which the gathers need for their
    // addresses) are fetched one pair ahead.
    auto sample_mem = [&](auto keyp, const float Pc[4], double (&a8)[8]) {
        const float A1 = 1.0f + Pc[0];
        uint32_t xy[2];
        auto load_xy = [&](int slot) {
#pragma unroll
            for (int u = 0; u < 2; u++) xy[u] = rxy[min(chunk_of(slot + u) * 64 + lane, end - 1)];
        };
        if (chunk_of(0) < nchunk) load_xy(0);
        for (int slot = 0; chunk_of(slot) < nchunk; slot += 2) {
            f32x4 jf[2];
            float tv[2];
            LanczosFetch f[2];
            int r[2];
#pragma unroll
            for (int u = 0; u < 2; u++) {
                r[u] = chunk_of(slot + u) * 64 + lane;
                const int rc2 = min(r[u], end - 1);
                jf[u] = rj[rc2];
                tv[u] = rtv[rc2];
                const float ox = (float)(xy[u] & 0xffffu), oy = (float)(xy[u] >> 16);
                f[u] = lanczos_fetch(keyp, w, h, w, A1 * ox - Pc[1] * oy + Pc[2], Pc[1] * ox + A1 * oy + Pc[3]);
            }
            if (chunk_of(slot + 2) < nchunk) load_xy(slot + 2);
#pragma unroll
            for (int u = 0; u < 2; u++) residual_terms(r[u], jf[u], tv[u] - lanczos_finish(f[u], w), a8);
        }
    };
    float P[4];
    ul_params_sparse(T, w, h, P);
    auto solve_hessian = [&]() {      // wave 0: alignment.cpp:555-583
        double hacc[10];
#pragma unroll
        for (int k = 0; k < 10; k++) {
            double t = 0.0;
            for (int wv = 0; wv < kWaves; wv++) t += sh.red[0][wv * 10 + k];
            hacc[k] = t;
        }
        double H[16], Hinv[16];
        int k = 0;
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int b = a; b < 4; b++) { H[a * 4 + b] = hacc[k]; H[b * 4 + a] = hacc[k]; k++; }
        const double cond = condition_and_invert(H, Hinv);
        double c1[8];
        warp_corners(T, w, h, c1);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int i = 0; i < 16; i++) sh.hinv[i] = Hinv[i];
            sh.hinv[16] = cond;
#pragma unroll
            for (int i = 0; i < 8; i++) { sh.c0[i] = c1[i]; sh.c1[i] = c1[i]; }
        }
    };
    const double scale = 1.0 / w;   // alignment.cpp:629
    // dt = Hinv b, delta.compose(T) (alignment.cpp:629-639) from the per-wave partial sums of the sampler waves.  Runs on
    // wave 0 with the samplers waiting for the result, so it is laid across the lanes to keep the dependent chain short:
    // lane 8 (v - first) + c reads component c of wave v, a fixed tree of pairs of waves adds them, lanes
    // 0..3 form b[c] = (x-set + y-set) / 2 and one row of Hinv b each, and every lane composes the new transform.
    auto lane_bcast = [](double x, int src) -> double {
        return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), src), __builtin_amdgcn_readlane(__double2loint(x), src));
    };
    // first_wave: 1 = the sampler waves' sums of a pass; 0 = every wave's sums (the first pass of a level, summed from the
    // records' residuals while they were written: gn_hessian_partials / the fused kernel's gather)
    auto next_transform = [&](const VS_LDS_AS double* red, int first_wave, const double Tc[4], double Tn[4]) {
        const int n_vals = (kWaves - first_wave) * 8;
        double v = 0.0;
#pragma unroll
        for (int g = 0; g * 64 < kWaves * 8; g++) {
            const int idx = lane + 64 * g;
            if (idx < n_vals) v += red[8 * first_wave + idx];
        }
        v = v + dpp_mov_keep<0x108>(0.0, v);                        // + the lane 8 up in the row (row_shl:8; lanes 8..15: unused)
        {
            const int lo = __builtin_amdgcn_ds_swizzle(__double2loint(v), (0x10 << 10) | 0x1f);
            const int hi = __builtin_amdgcn_ds_swizzle(__double2hiint(v), (0x10 << 10) | 0x1f);
            v = v + __hiloint2double(hi, lo);                       // + the neighbouring row
        }
        {
            const int src = (lane ^ 32) << 2;
            const int lo = __builtin_amdgcn_ds_bpermute(src, __double2loint(v));
            const int hi = __builtin_amdgcn_ds_bpermute(src, __double2hiint(v));
            v = v + __hiloint2double(hi, lo);                       // + the other half: lanes 0..7 hold the eight sums
        }
        const double bc = (v + dpp_mov_keep<0x104>(0.0, v)) * 0.5f;    // lanes 0..3: (sx + sy) * 0.5 (generators.cpp:595)
        const double b0 = lane_bcast(bc, 0), b1 = lane_bcast(bc, 1), b2 = lane_bcast(bc, 2), b3 = lane_bcast(bc, 3);
        const int r = lane & 3;
        double dtr = 0.0;
        dtr += sh.hinv[r * 4 + 0] * b0;
        dtr += sh.hinv[r * 4 + 1] * b1;
        dtr += sh.hinv[r * 4 + 2] * b2;
        dtr += sh.hinv[r * 4 + 3] * b3;
        const double delta[4] = {lane_bcast(dtr, 0) * scale, lane_bcast(dtr, 1) * scale, lane_bcast(dtr, 2), lane_bcast(dtr, 3)};
        compose(delta, Tc, Tn);
    };
    // corner test of alignment.cpp:641-677 on wave 0: 0 iterate on / 1 converged / 2 out of iterations / 3 over max_displacement
    auto corner_test = [&](const double Tn[4], int iter) -> int {
        double c1[8], c2[8];
#pragma unroll
        for (int i = 0; i < 8; i++) c1[i] = sh.c1[i];      // wave 0 only: LDS accesses of one wave are in program order
        warp_corners(Tn, w, h, c2);
        const double disp12 = corner_move(c2, c1);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int i = 0; i < 8; i++) sh.c1[i] = c2[i];
        }
        int f = 0;
        if (disp12 < threshold) f = 1;
        else if (iter >= max_iters - 1) f = 2;
        if (f == 1) {   // alignment.cpp:670-677: total corner move of the level
            double c0[8];
#pragma unroll
            for (int i = 0; i < 8; i++) c0[i] = sh.c0[i];
            if (corner_move(c0, c2) > max_displacement) f = 3;
        }
        return f;
    };
    int iters = 0, flag = 0;
    // every chunk needs a register slot in its wave
    const bool pipelined = kVF == 1 && from_lds && max_iters > 0 && __builtin_amdgcn_readfirstlane(gp_in.pipeline) != 0 &&
                           (weighted || nchunk <= kRecChunks * (kWaves - 1));
    if (pipelined) {
        // Coarsest level (image in LDS, typically 10-20 iterations): an iteration costs ONE barrier.  After the barrier that
        // completes the partial sums of iteration k, wave 0 computes T(k+1) and publishes it straight away (sequence word,
        // no barrier); the samplers pick it up and sample iteration k+1 while wave 0 is still busy with the corner test of
        // iteration k.  Its verdict (ctl) is read after the next barrier: if the level is over, the sampling pass in flight
        // was speculative and is dropped (the samplers poll ctl between their pairs of chunks and leave early).  The same
        // operations on the same values as the two-barrier loop below.
        // The records of a wave's points do not change during the level: they are read into registers once, so the
        // iteration loop touches no global memory at all.
        uint32_t rxyc[kRecChunks];
        float rtvc[kRecChunks];
        f32x4 rjc[kRecChunks];
#pragma unroll
        for (int j = 0; j < kRecChunks; j++) {
            const int r = max(min(chunk_of(j) * 64 + lane, end - 1), 0);         // (wave 0 has no chunks: clamped, unused)
            rxyc[j] = rxy[r]; rtvc[j] = rtv[r]; rjc[j] = rj[r];
        }
        auto sample_regs = [&](const float Pc[4], double (&a8)[8], int poll_iter) {
            const float A1 = 1.0f + Pc[0];
#pragma unroll
            for (int j = 0; j < kRecChunks; j += 2) {
                if (chunk_of(j) >= nchunk) break;
                LanczosFetch f[2];
#pragma unroll
                for (int u = 0; u < 2; u++) {
                    const float ox = (float)(rxyc[j + u] & 0xffffu), oy = (float)(rxyc[j + u] >> 16);
                    f[u] = lanczos_fetch(lkey, w, h, w, A1 * ox - Pc[1] * oy + Pc[2], Pc[1] * ox + A1 * oy + Pc[3]);
                }
#pragma unroll
                for (int u = 0; u < 2; u++)
                    residual_terms(chunk_of(j + u) * 64 + lane, rjc[j + u], rtvc[j + u] - lanczos_finish(f[u], w), a8);
                if (poll_iter > 0) {
                    const int v = __hip_atomic_load(&sh.ctl[(poll_iter - 1) & 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if ((v >> 2) == poll_iter && (v & 3) != 0) break;     // the level ended with the previous iteration
                }
            }
        };
        if (threadIdx.x == 0) { sh.seq = 0; sh.ctl[0] = 0; sh.ctl[1] = 0; }
        // iteration 0 needs no sampling: its sums are in red[1] already (all waves'); wave 0 solves the 4x4 problem (red[0]).
        if (w0) solve_hessian();
        __syncthreads();
        for (int k = 0;; k++) {
            // the partial sums of iteration k are in red[(k + 1) & 1]; those of k + 1 go to red[k & 1]
            if (w0) {
                double Tn[4];
                next_transform(sh.red[(k + 1) & 1], k == 0 ? 0 : 1, T, Tn);
                if (threadIdx.x == 0) {
                    VS_LDS_AS double* Tp = sh.Tp[k & 1];
                    Tp[0] = Tn[0]; Tp[1] = Tn[1]; Tp[2] = Tn[2]; Tp[3] = Tn[3];
                    __hip_atomic_store(&sh.seq, k + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
                const int f = corner_test(Tn, k);
                if (threadIdx.x == 0) __hip_atomic_store(&sh.ctl[k & 1], ((k + 1) << 2) | f, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            } else {
                while (__hip_atomic_load(&sh.seq, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != k + 1) __builtin_amdgcn_s_sleep(1);
                const VS_LDS_AS double* Tp = sh.Tp[k & 1];
                const double Ts[4] = {Tp[0], Tp[1], Tp[2], Tp[3]};
                float Ps[4];
                ul_params_sparse(Ts, w, h, Ps);
                double a8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                sample_regs(Ps, a8, k + 1);
                wave_partials8_butterfly(a8, sh.red[k & 1], wave);
            }
            __syncthreads();
            T[0] = sh.Tp[k & 1][0]; T[1] = sh.Tp[k & 1][1]; T[2] = sh.Tp[k & 1][2]; T[3] = sh.Tp[k & 1][3];
            flag = sh.ctl[k & 1] & 3;
            iters = k + 1;
            if (flag) break;
        }
    } else {
        // Two barriers per iteration: [samplers: partial sums] barrier [wave 0: transform update + corner test] barrier.
        // Iteration 0 needs no sampling (its sums are in red[1] already, all waves'); the Hessian partials are in red[0] until
        // wave 0 has read them.
        if (w0) solve_hessian();
        for (int iter = 0; iter < max_iters; iter++) {
            iters++;
            VS_LDS_AS double* red = sh.red[iter == 0 ? 1 : 0];
            if (!w0 && iter > 0) {
                ul_params_sparse(T, w, h, P);
                for (int vn = 0; vn < (kVF == 1 ? 1 : 3); vn++) {
                    wave = __builtin_amdgcn_readfirstlane(vwave_of(vn));
                    if (wave < 0) break;
                    double a8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                    if (from_lds) sample_mem(lkey, P, a8); else sample_mem(gkey, P, a8);
                    wave_partials8_butterfly(a8, red, wave);
                }
            }
            __syncthreads();
            if (w0) {
                double Tn[4];
                next_transform(red, iter == 0 ? 0 : 1, T, Tn);
                const int f = corner_test(Tn, iter);
                if (threadIdx.x == 0) {
                    sh.T[0] = Tn[0]; sh.T[1] = Tn[1]; sh.T[2] = Tn[2]; sh.T[3] = Tn[3];
                    sh.flag = f;
                }
            }
            __syncthreads();
            T[0] = sh.T[0]; T[1] = sh.T[1]; T[2] = sh.T[2]; T[3] = sh.T[3];
            flag = sh.flag;
            if (flag) break;
        }
    }
    const int fail = flag == 1 ? 0 : flag;
    if (!fail && level > 0) { T[2] *= 2.0; T[3] *= 2.0; }   // alignment.cpp:683-687
    T_io[0] = T[0]; T_io[1] = T[1]; T_io[2] = T[2]; T_io[3] = T[3];
    *iters_out = iters;
    *cond_out = sh.hinv[16];
    __syncthreads();   // sh.T / sh.flag / sh.red are rewritten by the next level
    return fail;
}

// Per-level form (selection on the host between launches: VS_SELECT_STL_HOST)
__global__ VS_GN_FUSED_BOUNDS __attribute__((unused)) void vs_k_gn_level(PairState* __restrict__ states,
                                                            const PairDesc* __restrict__ descs,
                                                            const uint8_t* __restrict__ pyr, size_t pyr_frame,
                                                            size_t img_off, int w, int h, int nsel,
                                                            uint8_t* __restrict__ recs, size_t recs_pair, int nt_cap,
                                                            int level, GnParams gp) {
    __shared__ GnShared sh;
    const int p = blockIdx.x;
    PairState& st = states[p];
    if (st.status != 1) return;   // uniform for the block
    const PairDesc d = descs[p];
    const uint8_t* key = pyr + (size_t)d.key_slot * pyr_frame + img_off;
    const PointRecs rc = pair_recs(recs, recs_pair, p, nt_cap);
    double T[4] = {st.T[0], st.T[1], st.T[2], st.T[3]};
    int iters;
    double cond;
    gn_hessian_partials(sh, rc, nsel);
    __syncthreads();
    const int fail = gn_level(sh, key, nullptr, w, h, nsel, rc, level, gp, T, &iters, &cond);
    __syncthreads();   // every thread has read st.T before thread 0 rewrites it
    if (threadIdx.x == 0) {
        st.iterations[level] = iters;
        st.condition[level] = cond;
        if (fail != 2) {     // the estimate the level ended on, before gn_level's x2 of TX,TY (halving undoes it exactly)
            const double u = (!fail && level > 0) ? 0.5 : 1.0;
            st.level_T[level][0] = T[0]; st.level_T[level][1] = T[1]; st.level_T[level][2] = T[2] * u; st.level_T[level][3] = T[3] * u;
        }
        if (fail) { st.status = 0; st.fail_reason = fail; st.fail_level = level; }
        st.T[0] = T[0]; st.T[1] = T[1]; st.T[2] = T[2]; st.T[3] = T[3];
    }
}

// ---- on-device replica of libstdc++'s std::nth_element (bits/stl_algo.h, GCC 11) -----------------
// alignment.cpp:466-486 calls std::nth_element(begin, begin+n, end, abs_delta <) and keeps the first
// n elements.  Which tied elements survive, and in which order, is decided by libstdc++'s
// __introselect: median-of-3 (first+1, mid, last-1) moved to `first`, an unguarded Hoare partition of
// [first+1,last) around it, recurse into the side holding nth, insertion sort once <= 3 remain.
// The Hoare sweep is sequential in the STL but depends only on the ORIGINAL values: its k-th swap
// exchanges the k-th left stopper (a[i] >= pivot, scanning up) with the k-th right stopper
// (a[j] <= pivot, scanning down) for as long as the former lies left of the latter, and it returns
// the first left stopper that did not swap (or the last right stopper that did).  That is a pair of
// prefix counts, so one partition is a few block-wide scans.  tests/test_select_gpu.py checks the
// permutation against the host's std::nth_element on tie-heavy inputs.
// Elements are packed (abs_delta << 16) | tile_index; only abs_delta takes part in comparisons.
// selection tuning (tools/select_bench.py): ranges up to kWaveRange elements are finished by one wave; the
// block-wide rounds give elements to kSelThreadsSmall threads (more only when a 32-element chunk would not cover the range)
constexpr int kWaveRange = 256, kSelThreadsSmall = 256;
struct SelShared {
    int wl[kGnThreads / 64], wr[kGnThreads / 64];   // per-wave stopper counts
    int red_k[kGnThreads / 64], red_c[kGnThreads / 64];
    // introselect_regs' two 64-byte rank tables.  They used to borrow the first 128 bytes of the caller's posR array, which holds only 2 * n
    // bytes: with fewer than 64 tiles per set (a 20 x 13 top level) the x-set's second table ran into the y-set's first one in the side-by-side
    // layout of introselect_dual (aX | aY | posRX | posRY), the two waves working at the same time.  Found by the bounds-checked build's random
    // sweep (round 4, case 48: the debug build's timing made the collision visible; the regular build had been getting away with it).
    __attribute__((aligned(16))) uint8_t tab[128];
};

// One wave finishes the job once the active range fits 64 lanes x 32 elements: the same partition rounds,
// but every exchange is a wave shuffle and LDS accesses of a single wave execute in program order, so a round
// costs no block barrier (most rounds of an introselect run are on small ranges: the block-wide rounds take
// ~1.7 us each, these ~0.3 us).  Called by wave 0 only, with all 64 lanes.
// The selection arrays live in LDS.  The functions below are not inlined, so their pointer arguments arrive generic (every
// access a flat_load / flat_store) and their scalars per lane; each function re-types them on entry: address space 3 for
// the arrays (ds_read / ds_write), readfirstlane for the wave-uniform scalars.
typedef VS_LDS_AS uint32_t lds_u32;
typedef VS_LDS_AS uint16_t lds_u16;
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

__device__ __forceinline__ void median_to_first(VS_ARR(lds_u32*) a, int first, int last) {
    // __unguarded_partition_pivot: __move_median_to_first(first, first+1, mid, last-1)
    const int mid = first + (last - first) / 2;
    const int ia = first + 1, ib = mid, ic = last - 1;
    const uint32_t A = a[ia] >> 16, B = a[ib] >> 16, C = a[ic] >> 16;
    int m;
    if (A < B) m = (B < C) ? ib : ((A < C) ? ic : ia);
    else if (A < C) m = ia;
    else if (B < C) m = ic;
    else m = ib;
    const uint32_t t = a[first]; a[first] = a[m]; a[m] = t;
}

// The last rounds, once the range is at most 64 elements: one element per lane, in a register.  A partition round is then
// two ballots (left / right stoppers), their ranks from mbcnt / popcount, one trip through two 64-byte LDS tables to find
// the partner (rank r from the left pairs with rank r from the right) and one ds_bpermute to exchange the values -- no
// per-lane loops, no dependent LDS chains (~500 cycles per round against ~1700 for the chunked form below).  Same pivots,
// same swaps, same cut as introselect_wave; the final insertion sort runs on the array in LDS as there.
// `tab`: 128 bytes of LDS scratch of this selection's own (SelShared::tab).  Returns the remaining depth (>= 0), or -1 when the depth
// limit was hit; *first_io / *last_io = the range left for the insertion sort.
__device__ __forceinline__ int introselect_regs(VS_ARR(lds_u32*) a, VS_LDS_AS uint8_t* __restrict__ tab, int* first_io, int* last_io, int nth,
                                                int depth) {
    const int lane = threadIdx.x & 63;
    const int base = *first_io, m0 = *last_io - base;            // relative index = lane
    VS_SPAN(VS_LDS_AS uint8_t*, posRt, tab, 64, 101);
    VS_SPAN(VS_LDS_AS uint8_t*, posLt, tab + 64, 64, 102);
    uint32_t v = lane < m0 ? a[base + lane] : 0u;
    int f = 0, l = m0;
    const int nthr = nth - base;
    auto lane_val = [&](int src) -> uint32_t { return (uint32_t)__builtin_amdgcn_readlane((int)v, src); };
    while (l - f > 3) {
        if (depth == 0) { depth = -1; break; }
        --depth;
        // __unguarded_partition_pivot: __move_median_to_first(first, first+1, mid, last-1)
        const int ia = f + 1, ib = f + (l - f) / 2, ic = l - 1;
        const uint32_t A = lane_val(ia) >> 16, B = lane_val(ib) >> 16, C = lane_val(ic) >> 16;
        int m;
        if (A < B) m = (B < C) ? ib : ((A < C) ? ic : ia);
        else if (A < C) m = ia;
        else if (B < C) m = ic;
        else m = ib;
        const uint32_t vf = lane_val(f), vm = lane_val(m);
        v = lane == f ? vm : (lane == m ? vf : v);
        const uint32_t pv = vm >> 16;
        const bool in = lane > f && lane < l;
        const uint32_t k = v >> 16;
        const bool L = in && k >= pv, R = in && k <= pv;
        const unsigned long long bL = __ballot(L), bR = __ballot(R);
        const int nR = __popcll(bR);
        const int rankL = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bL >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bL, 0u));
        const int rankR = __popcll((bR >> lane) >> 1);                     // right stoppers above this lane
        if (R) posRt[rankR] = (uint8_t)lane;
        if (L) posLt[rankL] = (uint8_t)lane;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const int j = (L && rankL < nR) ? (int)posRt[rankL] : -1;          // my partner when I am a left stopper
        const bool swapL = L && lane < j;
        const unsigned long long bS = __ballot(swapL), bN = __ballot(L && !swapL);
        const int K = __popcll(bS);
        const bool swapR = R && rankR < K;                                  // (a lane never swaps in both roles)
        const int i_for_r = swapR ? (int)posLt[rankR] : lane;
        const int src = swapL ? j : i_for_r;
        const uint32_t got = (uint32_t)__builtin_amdgcn_ds_bpermute(src << 2, (int)v);
        if (swapL || swapR) v = got;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const int cand = bN ? (int)__ffsll((long long)bN) - 1 : 0x7fffffff;
        const int RK = K > 0 ? __builtin_amdgcn_readfirstlane((int)posRt[K - 1]) : l;
        const int cut = (cand != 0x7fffffff && cand < RK) ? cand : RK;
        if (cut <= nthr) f = cut; else l = cut;
    }
    if (lane < m0) a[base + lane] = v;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    *first_io = base + f; *last_io = base + l;
    return depth;
}

__device__ __noinline__ int introselect_wave(uint32_t* __restrict__ a_g, uint16_t* __restrict__ posR_g, uint8_t* __restrict__ tab_g, int first, int last,
                                             int nth, int depth) {
    VS_SPAN(lds_u32*, a, a_g, uni(last), 103);            // (the range only ever shrinks: [first, last) of the call bounds every access)
    VS_SPAN(lds_u16*, posR, posR_g, uni(last) - uni(first), 104);     // ranks of right stoppers: fewer than the range has elements
    VS_LDS_AS uint8_t* const tab = (VS_LDS_AS uint8_t*)tab_g;
    first = uni(first); last = uni(last); nth = uni(nth); depth = uni(depth);
    const int lane = threadIdx.x & 63;
    while (last - first > 3) {
        if (last - first <= 64) {                         // the rest in registers
            depth = introselect_regs(a, tab, &first, &last, nth, depth);
            if (depth < 0) return 1;
            break;
        }
        if (depth == 0) return 1;
        --depth;
        if (lane == 0) median_to_first(a, first, last);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const uint32_t pv = a[first] >> 16;
        const int f0 = first + 1, m = last - f0;
        const int chunk = (m + 63) >> 6;                  // <= 32
        const int lo = min(f0 + lane * chunk, last), hi = min(lo + chunk, last);
        uint32_t maskL = 0, maskR = 0;
        for (int i = lo; i < hi; i++) {
            const uint32_t k = a[i] >> 16;
            maskL |= (uint32_t)(k >= pv) << (i - lo);
            maskR |= (uint32_t)(k <= pv) << (i - lo);
        }
        const int cl = __popc(maskL), cr = __popc(maskR);
        const int il = wave_incl_scan(cl), ir = wave_incl_scan(cr);
        const int nR = wave_total(ir);
        {
            int rk = nR - ir;
            uint32_t mr = maskR;
            while (mr) {
                const int e = 31 - __clz(mr);
                mr &= ~(1u << e);
                posR[rk++] = (uint16_t)(lo + e);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        int swaps = 0, cand = 0x7fffffff;
        {
            int k = il - cl;
            uint32_t ml = maskL;
            while (ml) {
                const int e = __ffs(ml) - 1;
                ml &= ml - 1;
                const int i = lo + e;
                const int j = k < nR ? (int)posR[k] : -1;
                if (i < j) { const uint32_t t = a[i]; a[i] = a[j]; a[j] = t; swaps++; }
                else if (cand == 0x7fffffff) cand = i;
                k++;
            }
        }
        swaps = wave_total(wave_incl_scan(swaps));
        cand = wave_min_nonneg(cand);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const int RK = swaps > 0 ? (int)posR[swaps - 1] : last;
        const int cut = (cand != 0x7fffffff && cand < RK) ? cand : RK;
        if (cut <= nth) first = cut; else last = cut;
    }
    // __insertion_sort(first, last) on <= 3 elements
    if (lane == 0) {
        for (int i = first + 1; i < last; i++) {
            const uint32_t v = a[i];
            if ((v >> 16) < (a[first] >> 16)) {
                for (int j = i; j > first; j--) a[j] = a[j - 1];
                a[first] = v;
            } else {
                int j = i;
                while ((v >> 16) < (a[j - 1] >> 16)) { a[j] = a[j - 1]; j--; }
                a[j] = v;
            }
        }
    }
    return 0;
}

// returns 0 on success, 1 when libstdc++ would have fallen back to heap-select (depth limit): the
// caller then re-runs the pair through the host path.
__device__ __noinline__ int introselect_block(uint32_t* __restrict__ a_g, uint16_t* __restrict__ posR_g, SelShared& ss_g,
                                              int n, int nth, int depth_cap = 0) {
    VS_SPAN(lds_u32*, a, a_g, uni(n), 105);
    VS_SPAN(lds_u16*, posR, posR_g, uni(n), 106);
    VS_LDS_AS SelShared& ss = *(VS_LDS_AS SelShared*)&ss_g;
    n = uni(n); nth = uni(nth);
    if (n == 0 || nth == n) return 0;                 // std::nth_element's early return
    int first = 0, last = n;
    int depth = 2 * (31 - __clz(n));                  // std::__lg(n) * 2
    depth_cap = uni(depth_cap);
    if (depth_cap > 0) depth = min(depth, depth_cap); // test hook (GnParams::sel_depth_cap)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    bool fail = false;
    // block-wide rounds while the range is large.  Round structure: [median swap by thread 0] barrier
    // [classify + count] barrier [rank table] barrier [swaps + reduce] barrier; the next round's median swap
    // rides in front of the following barrier.
    bool median_done = false;
    while (last - first > 3 && last - first - 1 > kWaveRange) {
        if (depth == 0) { fail = true; break; }
        --depth;
        if (!median_done) {
            if (tid == 0) median_to_first(a, first, last);
            __syncthreads();
        }
        const uint32_t pv = a[first] >> 16;
        const int f0 = first + 1, m = last - f0;
        // kSelThreadsSmall threads own elements, unless a 32-element chunk per thread would not cover the range; then every thread of the block takes part, with
        // chunks of up to 64 elements (the masks are 64 bits wide)
        const int kSelThreads = m > 32 * kSelThreadsSmall ? kGnThreads : kSelThreadsSmall;
        const int chunk = (m + kSelThreads - 1) / kSelThreads;   // <= 64: the caller caps n at 64*kGnThreads
        const int lo = min(f0 + min(tid, kSelThreads) * chunk, last), hi = tid < kSelThreads ? min(lo + chunk, last) : lo;
        // classify my chunk once, from the unmodified values: bit e of maskL / maskR = element lo+e stops the
        // left / right scan.  Later passes use only the masks, so swaps by other threads cannot disturb them.
        uint64_t maskL = 0, maskR = 0;
        for (int i = lo; i < hi; i++) {
            const uint32_t k = a[i] >> 16;
            maskL |= (uint64_t)(k >= pv) << (i - lo);
            maskR |= (uint64_t)(k <= pv) << (i - lo);
        }
        const int cl = __popcll(maskL), cr = __popcll(maskR);
        const int il = wave_incl_scan(cl), ir = wave_incl_scan(cr);
        if (lane == 63) { ss.wl[wave] = il; ss.wr[wave] = ir; }
        __syncthreads();
        int pre_l = il - cl, pre_r_incl = ir, nR = 0;
        for (int wv = 0; wv < kSelThreads / 64; wv++) {
            const int a_l = ss.wl[wv], a_r = ss.wr[wv];
            if (wv < wave) { pre_l += a_l; pre_r_incl += a_r; }
            nR += a_r;
        }
        // right-stopper ranks count from the right: rank of my topmost stopper = # stoppers after my chunk
        {
            int rk = nR - pre_r_incl;
            uint64_t mr = maskR;
            while (mr) {
                const int e = 63 - __clzll((long long)mr);
                mr &= ~(1ull << e);
                posR[rk++] = (uint16_t)(lo + e);
            }
        }
        __syncthreads();
        // left stoppers in increasing order: rank k swaps with posR[k] while it lies to the left of it.
        // Swapped pairs are disjoint (every swapping left stopper is left of every swapping right stopper).
        int swaps = 0, cand = 0x7fffffff;
        {
            int k = pre_l;
            uint64_t ml = maskL;
            while (ml) {
                const int e = __ffsll((long long)ml) - 1;
                ml &= ml - 1;
                const int i = lo + e;
                const int j = k < nR ? (int)posR[k] : -1;
                if (i < j) { const uint32_t t = a[i]; a[i] = a[j]; a[j] = t; swaps++; }
                else if (cand == 0x7fffffff) cand = i;
                k++;
            }
        }
        // K = total swaps; cand = position of the first left stopper that did not swap
        swaps = wave_total(wave_incl_scan(swaps));
        cand = wave_min_nonneg(cand);
        if (lane == 0) { ss.red_k[wave] = swaps; ss.red_c[wave] = cand; }
        __syncthreads();
        int K = 0, c = 0x7fffffff;
        for (int wv = 0; wv < kSelThreads / 64; wv++) { K += ss.red_k[wv]; c = min(c, ss.red_c[wv]); }
        const int RK = K > 0 ? (int)posR[K - 1] : last;
        const int cut = (c != 0x7fffffff && c < RK) ? c : RK;
        if (cut <= nth) first = cut; else last = cut;
        // every swap of this round is complete (barrier above): thread 0 may already place the next round's
        // pivot; the barrier that closes this round (posR / ss are rewritten next) then also publishes it
        median_done = false;
        if (last - first > 3 && last - first - 1 > kWaveRange && depth > 0) {
            if (tid == 0) median_to_first(a, first, last);
            median_done = true;
        }
        __syncthreads();
    }
    // the rest (including the final insertion sort) on one wave
    if (!fail && wave == 0) {
        if (introselect_wave(a_g, posR_g, ss_g.tab, first, last, nth, depth)) ss.red_k[0] = -1; else ss.red_k[0] = 0;
    }
    __syncthreads();
    return fail || ss.red_k[0] < 0 ? 1 : 0;
}

// The same selection with the arrays in GLOBAL memory (the pair's own scratch, L2-resident) for levels whose 6 B x tiles do
// not fit the workgroup's LDS: the small-footprint build at a 4K level 0 (20736 tiles per set: 124 KB against ~31 KB).  Same
// rounds, same pivots, same swaps, same cut as introselect_block -- the permutation is a function of the values alone -- with
// * up to 128 elements per thread (two 64-bit masks per side), so that 256 threads cover 32768 elements;
// * a thread's loads issued in batches of eight (every access is an L2 round trip; nothing else hides it);
// * the tail (<= kWaveRange + 1 elements) copied into `lds_tail` (>= 6 B x (kWaveRange + 1) bytes of LDS), finished
//   there by introselect_wave, and copied back.
// Stores of one thread are read by other threads of the workgroup only behind a workgroup barrier (which waits for vmcnt),
// on the same CU (same L1): the pattern the record arrays of the fused kernel already use.
typedef VS_GLOBAL_AS uint32_t glb_u32;
typedef VS_GLOBAL_AS uint16_t glb_u16;
__device__ __noinline__ int introselect_block_g(uint32_t* __restrict__ a_g, uint16_t* __restrict__ posR_g, SelShared& ss_g,
                                                uint32_t* lds_tail_g, int n, int nth, int depth_cap = 0) {
    VS_SPAN(glb_u32*, a, uniform_ptr(a_g), uni(n), 107);
    VS_SPAN(glb_u16*, posR, uniform_ptr(posR_g), uni(n), 108);
    VS_LDS_AS SelShared& ss = *(VS_LDS_AS SelShared*)&ss_g;
    n = uni(n); nth = uni(nth);
    if (n == 0 || nth == n) return 0;                 // std::nth_element's early return
    int first = 0, last = n;
    int depth = 2 * (31 - __clz(n));                  // std::__lg(n) * 2
    depth_cap = uni(depth_cap);
    if (depth_cap > 0) depth = min(depth, depth_cap); // test hook (GnParams::sel_depth_cap)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    bool fail = false;
    auto median_to_first_g = [&](int f, int l) {      // __move_median_to_first(first, first+1, mid, last-1), thread 0
        const int mid = f + (l - f) / 2, ia = f + 1, ib = mid, ic = l - 1;
        const uint32_t va = a[ia], vb = a[ib], vc = a[ic], vf = a[f];
        const uint32_t A = va >> 16, B = vb >> 16, C = vc >> 16;
        int m; uint32_t vm;
        if (A < B) { if (B < C) { m = ib; vm = vb; } else if (A < C) { m = ic; vm = vc; } else { m = ia; vm = va; } }
        else if (A < C) { m = ia; vm = va; }
        else if (B < C) { m = ic; vm = vc; }
        else { m = ib; vm = vb; }
        a[f] = vm; a[m] = vf;
    };
    bool median_done = false;
    while (last - first > 3 && last - first - 1 > kWaveRange) {
        if (depth == 0) { fail = true; break; }
        --depth;
        if (!median_done) {
            if (tid == 0) median_to_first_g(first, last);
            __syncthreads();
        }
        const uint32_t pv = a[first] >> 16;
        const int f0 = first + 1, m = last - f0;
        const int chunk = (m + kGnThreads - 1) / kGnThreads;        // <= 128: the caller caps n at 128 * kGnThreads
        const int lo = min(f0 + tid * chunk, last), hi = min(lo + chunk, last);
        // classify my chunk once, from the unmodified values: bit e of maskL / maskR[e >> 6] = element lo + e stops the left / right scan
        uint64_t maskL[2] = {0, 0}, maskR[2] = {0, 0};
        for (int b = lo; b < hi; b += 8) {
            uint32_t v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) v[u] = a[min(b + u, hi - 1)];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int e = b + u - lo;
                if (b + u < hi) {
                    const uint32_t k = v[u] >> 16;
                    maskL[e >> 6] |= (uint64_t)(k >= pv) << (e & 63);
                    maskR[e >> 6] |= (uint64_t)(k <= pv) << (e & 63);
                }
            }
        }
        const int cl = __popcll(maskL[0]) + __popcll(maskL[1]), cr = __popcll(maskR[0]) + __popcll(maskR[1]);
        const int il = wave_incl_scan(cl), ir = wave_incl_scan(cr);
        if (lane == 63) { ss.wl[wave] = il; ss.wr[wave] = ir; }
        __syncthreads();
        int pre_l = il - cl, pre_r_incl = ir, nR = 0;
        for (int wv = 0; wv < kRWaves; wv++) {
            const int a_l = ss.wl[wv], a_r = ss.wr[wv];
            if (wv < wave) { pre_l += a_l; pre_r_incl += a_r; }
            nR += a_r;
        }
        // right-stopper ranks count from the right: rank of my topmost stopper = # stoppers after my chunk
        {
            int rk = nR - pre_r_incl;
            for (int h = 1; h >= 0; h--) {
                uint64_t mr = maskR[h];
                while (mr) {
                    const int e = 63 - __clzll((long long)mr);
                    mr &= ~(1ull << e);
                    posR[rk++] = (uint16_t)(lo + 64 * h + e);
                }
            }
        }
        __syncthreads();
        // left stoppers in increasing order: rank k swaps with posR[k] while it lies to the left of it (disjoint pairs)
        int swaps = 0, cand = 0x7fffffff;
        {
            int k = pre_l;
            for (int h = 0; h < 2; h++) {
                uint64_t ml = maskL[h];
                while (ml) {
                    const int e = __ffsll((long long)ml) - 1;
                    ml &= ml - 1;
                    const int i = lo + 64 * h + e;
                    const int j = k < nR ? (int)posR[k] : -1;
                    if (i < j) { const uint32_t t = a[i], u = a[j]; a[i] = u; a[j] = t; swaps++; }
                    else if (cand == 0x7fffffff) cand = i;
                    k++;
                }
            }
        }
        swaps = wave_total(wave_incl_scan(swaps));
        cand = wave_min_nonneg(cand);
        if (lane == 0) { ss.red_k[wave] = swaps; ss.red_c[wave] = cand; }
        __syncthreads();
        int K = 0, c = 0x7fffffff;
        for (int wv = 0; wv < kRWaves; wv++) { K += ss.red_k[wv]; c = min(c, ss.red_c[wv]); }
        const int RK = K > 0 ? (int)posR[K - 1] : last;
        const int cut = (c != 0x7fffffff && c < RK) ? c : RK;
        if (cut <= nth) first = cut; else last = cut;
        median_done = false;
        if (last - first > 3 && last - first - 1 > kWaveRange && depth > 0) {
            if (tid == 0) median_to_first_g(first, last);
            median_done = true;
        }
        __syncthreads();
    }
    // the rest (including the final insertion sort) on one wave, on a copy of the active range in LDS
    if (!fail) {
        const int cnt = last - first;                                   // <= kWaveRange + 1
        VS_SPAN(lds_u32*, tl, lds_tail_g, kWaveRange + 1, 109);
        for (int i = tid; i < cnt; i += kGnThreads) tl[i] = a[first + i];
        __syncthreads();
        if (wave == 0) {
            const int r = introselect_wave(lds_tail_g, (uint16_t*)(lds_tail_g + (kWaveRange + 1)), ss_g.tab, 0, cnt, nth - first, depth);
            ss.red_k[0] = r ? -1 : 0;
        }
        __syncthreads();
        for (int i = tid; i < cnt; i += kGnThreads) a[first + i] = tl[i];
    }
    __syncthreads();
    return fail || ss.red_k[0] < 0 ? 1 : 0;
}

// Both point sets of a level at once: threads 0..511 select the x-set, threads 512..1023 the y-set, each half
// running the rounds of introselect_block on its own arrays.  The block barriers are shared, so the halves advance
// in lock step and a half that has finished its block-wide rounds idles through the other's; the wave-level tails
// then run side by side on wave 0 and wave 8.  Wall time = max instead of sum of the two selections.
__device__ __noinline__ int introselect_dual(uint32_t* __restrict__ aX, uint16_t* __restrict__ pRX, uint32_t* __restrict__ aY,
                                             uint16_t* __restrict__ pRY, SelShared* ss2, int n, int nth, int depth_cap = 0) {
    if (n == 0 || nth == n) return 0;                 // std::nth_element's early return (same n, nth for both sets)
    const int tid = threadIdx.x, half = tid / (kGnThreads / 2), gt = tid % (kGnThreads / 2), lane = tid & 63, gw = gt >> 6;
    n = uni(n); nth = uni(nth);
    uint32_t* a_g = half ? aY : aX;                   // uniform per wave (a half is 8 whole waves)
    uint16_t* posR_g = half ? pRY : pRX;
    VS_SPAN(lds_u32*, a, a_g, n, 110);
    VS_SPAN(lds_u16*, posR, posR_g, n, 111);
    VS_LDS_AS SelShared& ss = *(VS_LDS_AS SelShared*)&ss2[half];
    constexpr int kHalf = kGnThreads / 2, kHalfWaves = kHalf / 64;
    constexpr int kSmall = kSelThreadsSmall < kHalf ? kSelThreadsSmall : kHalf;
    int first = 0, last = n;
    int depth = 2 * (31 - __clz(n));
    depth_cap = uni(depth_cap);
    if (depth_cap > 0) depth = min(depth, depth_cap);   // test hook (GnParams::sel_depth_cap)
    bool fail = false;
    // does my half need another block-wide round?  if so take its depth token and place its pivot
    auto begin_round = [&]() -> bool {
        if (fail || !(last - first > 3 && last - first - 1 > kWaveRange)) return false;
        if (depth == 0) { fail = true; return false; }
        --depth;
        if (gt == 0) median_to_first(a, first, last);
        return true;
    };
    bool need = begin_round();
    while (__syncthreads_or(need)) {                 // also publishes the pivot swaps
        uint32_t maskL = 0, maskR = 0, pv = 0;
        int lo = 0, f0 = first + 1;
        if (need) {
            pv = a[first] >> 16;
            const int m = last - f0;
            const int nthr = m > 32 * kSmall ? kHalf : kSmall;      // a chunk must fit the 32-bit masks
            const int chunk = (m + nthr - 1) / nthr;
            lo = min(f0 + min(gt, nthr) * chunk, last);
            const int hi = gt < nthr ? min(lo + chunk, last) : lo;
            for (int i = lo; i < hi; i++) {
                const uint32_t k = a[i] >> 16;
                maskL |= (uint32_t)(k >= pv) << (i - lo);
                maskR |= (uint32_t)(k <= pv) << (i - lo);
            }
        }
        const int cl = __popc(maskL), cr = __popc(maskR);
        const int il = wave_incl_scan(cl), ir = wave_incl_scan(cr);
        if (lane == 63) { ss.wl[gw] = il; ss.wr[gw] = ir; }
        __syncthreads();
        int pre_l = il - cl, pre_r_incl = ir, nR = 0;
        for (int wv = 0; wv < kHalfWaves; wv++) {
            const int a_l = ss.wl[wv], a_r = ss.wr[wv];
            if (wv < gw) { pre_l += a_l; pre_r_incl += a_r; }
            nR += a_r;
        }
        {
            int rk = nR - pre_r_incl;
            uint32_t mr = maskR;
            while (mr) {
                const int e = 31 - __clz(mr);
                mr &= ~(1u << e);
                posR[rk++] = (uint16_t)(lo + e);
            }
        }
        __syncthreads();
        int swaps = 0, cand = 0x7fffffff;
        {
            int k = pre_l;
            uint32_t ml = maskL;
            while (ml) {
                const int e = __ffs(ml) - 1;
                ml &= ml - 1;
                const int i = lo + e;
                const int j = k < nR ? (int)posR[k] : -1;
                if (i < j) { const uint32_t t = a[i]; a[i] = a[j]; a[j] = t; swaps++; }
                else if (cand == 0x7fffffff) cand = i;
                k++;
            }
        }
        swaps = wave_total(wave_incl_scan(swaps));
        cand = wave_min_nonneg(cand);
        if (lane == 0) { ss.red_k[gw] = swaps; ss.red_c[gw] = cand; }
        __syncthreads();
        if (need) {
            int K = 0, c = 0x7fffffff;
            for (int wv = 0; wv < kHalfWaves; wv++) { K += ss.red_k[wv]; c = min(c, ss.red_c[wv]); }
            const int RK = K > 0 ? (int)posR[K - 1] : last;
            const int cut = (c != 0x7fffffff && c < RK) ? c : RK;
            if (cut <= nth) first = cut; else last = cut;
        }
        need = begin_round();     // all swaps of this round completed before the barrier above
    }
    int r = 0;
    if (!fail && gw == 0) r = introselect_wave(a_g, posR_g, ss2[half].tab, first, last, nth, depth);
    if (gt == 0) ss.red_k[0] = (fail || r) ? -1 : 0;
    __syncthreads();
    return (ss2[0].red_k[0] < 0 || ss2[1].red_k[0] < 0) ? 1 : 0;
}

// ---- VS_SELECT_STABLE: the keep-best-fraction step under a documented, STL-independent rule ----------------------------
// (SURVEY 8(f) rank 1; oracle twin vso_select_smallest_stable.)  Keep the nsel tiles that are smallest by (abs_delta, tile
// index) -- ties on abs_delta go to the lower tile index -- in ascending TILE order.  Any conforming std::nth_element may
// produce this set; the order, which the reference leaves to the STL, is fixed.  No partition rounds: a histogram of the
// 16-bit abs_delta finds the cut value D and the number r of tiles with exactly D that are kept (one pass when every
// abs_delta is below 256, as for 8-bit sources; three in general), then one prefix sum over the tiles in index order
// places the survivors: position = #(abs_delta < D before it) + min(#(abs_delta == D before it), r).
// a_s[i] = abs_delta << 16 | i (warpdiff_fill's packing), read only; o_s[0 .. nsel) receives the survivors' tile indices (what
// gather_fill reads in this mode).  Both sets of a level in the same passes (nsets = 2) or one (nsets = 1; a1 / o1 unused).
// LDS: the arrays live in LDS (ds_read / ds_write); else in global memory (the small-footprint build's 4K level 0).
struct StableShared {
    uint32_t hist[2][128];                  // 256 bins of 16-bit counters per set (a level has at most 32768 tiles)
    unsigned long long wsum[kGnThreads / 64];
    uint32_t cut_d[2], cut_r[2], any_hi[2];
};

template <bool LDS>
__device__ __noinline__ void stable_select(uint32_t* __restrict__ a0_g, uint16_t* __restrict__ o0_g, uint32_t* __restrict__ a1_g,
                                           uint16_t* __restrict__ o1_g, int nsets, int nt, int nsel, StableShared& ss_g,
                                           uint8_t* lds_scratch = nullptr, int lds_scratch_bytes = 0) {
    typedef typename std::conditional<LDS, const lds_u32, const glb_u32>::type key_t;
    typedef typename std::conditional<LDS, lds_u16, VS_GLOBAL_AS uint16_t>::type out_t;
    VS_SPAN(key_t*, a0, (LDS ? (key_t*)(uintptr_t)__builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)a0_g) : (key_t*)uniform_ptr(a0_g)), uni(nt), 112);
    VS_SPAN(key_t*, a1, (LDS ? (key_t*)(uintptr_t)__builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)a1_g) : (key_t*)uniform_ptr(a1_g)), uni(nt), 113);
    VS_SPAN(out_t*, o0, (LDS ? (out_t*)(uintptr_t)__builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)o0_g) : (out_t*)uniform_ptr(o0_g)), uni(nt), 114);
    VS_SPAN(out_t*, o1, (LDS ? (out_t*)(uintptr_t)__builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)o1_g) : (out_t*)uniform_ptr(o1_g)), uni(nt), 115);
    // (not inlined: the shared block arrives as a generic reference -- say that it is LDS, see gn_level)
    VS_LDS_AS StableShared& ss = *(VS_LDS_AS StableShared*)(uintptr_t)__builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)&ss_g);
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    nsets = uni(nsets); nt = uni(nt); nsel = uni(nsel);
    if (nsel <= 0) return;                                                   // (uniform)
    // The abs_delta values of a level crowd into a few bins, so the lanes of a wave collide on the same counters (measured: 20 k
    // ticks for the 10368 keys of a 1080p level 0 on one histogram).  LDS arrays: the counting runs on up to eight lane-sliced
    // copies of the histogram (lane & (S - 1)) that live in the output area o_s -- dead until the placement, which starts
    // behind the barrier that ends the last use of the counters -- and are added up by the pick.  Packed 16-bit counters stay
    // carry-free in the sum too (a bin's total is at most nt <= 32768).
    // (copies 132 words apart: the same bin of the eight copies falls into eight different LDS banks)
    constexpr int kSub = 132;
    int S = 1;
    VS_LDS_AS uint32_t* hb0 = &ss.hist[0][0];
    VS_LDS_AS uint32_t* hb1 = &ss.hist[1][0];
    if (LDS) {
        const int room = (2 * nt - 2) / (4 * kSub);                          // whole padded histograms behind a 4-byte alignment
        const int s_fit = room >= 8 ? 8 : (room >= 4 ? 4 : (room >= 2 ? 2 : 0));
        if (s_fit) {
            S = s_fit;
            hb0 = (VS_LDS_AS uint32_t*)(((uintptr_t)(unsigned)(uintptr_t)VS_SPAN_RAW(o0) + 3u) & ~(uintptr_t)3u);
            hb1 = (VS_LDS_AS uint32_t*)(((uintptr_t)(unsigned)(uintptr_t)VS_SPAN_RAW(o1) + 3u) & ~(uintptr_t)3u);
        }
    }
    if (!LDS && nsets == 1 && lds_scratch != nullptr && lds_scratch_bytes >= 8 * 4 * kSub) {
        // (arrays in global memory: the level's LDS block is idle -- the copies of the one set's histogram go there)
        S = 8;
        hb0 = (VS_LDS_AS uint32_t*)(uintptr_t)__builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)lds_scratch);
    }
    const int sub = (lane & (S - 1)) * kSub;
    // (the histogram copies: S * kSub words behind hb0 / hb1 -- inside ss.hist, the output area or the idle level block)
    auto bump = [&](int s, uint32_t bin) {
        VS_BOUNDS_CHECK(sub + (int)(bin >> 1), S * kSub, 116);
        __hip_atomic_fetch_add((s ? hb1 : hb0) + sub + (bin >> 1), 1u << (16 * (bin & 1u)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    };
    auto clear_hist = [&]() {
        for (int s = 0; s < nsets; s++)
            for (int i = tid; i < S * kSub; i += kGnThreads) (s ? hb1 : hb0)[i] = 0u;
    };
    // wave s finds, in set s's histogram, the bin that holds the k-th smallest counted element (k >= 1) and how many of that
    // bin's elements are needed to get there: -> cut_d, cut_r
    auto scan_pick = [&](uint32_t k_of_set0, uint32_t k_of_set1) {
        if (wave < nsets) {
            const uint32_t k = wave ? k_of_set1 : k_of_set0;
            const VS_LDS_AS uint32_t* hb = wave ? hb1 : hb0;
            uint32_t w0 = 0u, w1 = 0u;
            for (int c2 = 0; c2 < S; c2++) { w0 += hb[c2 * kSub + 2 * lane]; w1 += hb[c2 * kSub + 2 * lane + 1]; }
            const uint32_t c[4] = {w0 & 0xffffu, w0 >> 16, w1 & 0xffffu, w1 >> 16};
            const uint32_t sum = c[0] + c[1] + c[2] + c[3];
            uint32_t inc = sum;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t up = (uint32_t)__shfl_up((int)inc, d, 64);
                if (lane >= d) inc += up;
            }
            uint32_t below = inc - sum;
            if (k > below && k <= inc) {                                     // exactly one lane
                int b = 0;
#pragma unroll
                for (int j = 0; j < 3; j++)
                    if (b == j && k > below + c[j]) { below += c[j]; b = j + 1; }
                ss.cut_d[wave] = (uint32_t)(4 * lane + b);
                ss.cut_r[wave] = k - below;
            }
        }
    };
    // every walk below loads kB keys before it uses the first (a loop of dependent LDS reads costs ~300 cycles per key)
    constexpr int kB = 8;
    auto walk_strided = [&](VS_ARR(key_t*) a, auto&& use) {                  // keys tid, tid + T, ...
        for (int i0 = tid; i0 < nt; i0 += kB * kGnThreads) {
            uint32_t v[kB];
#pragma unroll
            for (int u = 0; u < kB; u++) v[u] = a[min(i0 + u * kGnThreads, nt - 1)];
#pragma unroll
            for (int u = 0; u < kB; u++) if (i0 + u * kGnThreads < nt) use(v[u]);
        }
    };
    // ---- the cut: first on the assumption that every abs_delta is below 256 (one pass), else byte by byte
    if (tid < 2) ss.any_hi[tid] = 0u;
    clear_hist();
    __syncthreads();
    for (int s = 0; s < nsets; s++) {
        VS_SPAN(key_t*, a, VS_SPAN_RAW(s ? a1 : a0), nt, 117);
        bool seen = false;
        walk_strided(a, [&](uint32_t key) {
            const uint32_t d = key >> 16;
            if (d < 256u) bump(s, d);
            else seen = true;
        });
        if (__any(seen) && lane == 0) ss.any_hi[s] = 1u;
    }
    __syncthreads();
    const bool general = ss.any_hi[0] != 0u || (nsets > 1 && ss.any_hi[1] != 0u);     // (uniform)
    uint32_t hi0 = 0u, hi1 = 0u, k0 = (uint32_t)nsel, k1 = (uint32_t)nsel;
    if (general) {
        __syncthreads();                                                     // everyone has read any_hi and the first histogram
        clear_hist();
        __syncthreads();
        for (int s = 0; s < nsets; s++) {
            VS_SPAN(key_t*, a, VS_SPAN_RAW(s ? a1 : a0), nt, 117);
            walk_strided(a, [&](uint32_t key) { bump(s, key >> 24); });
        }
        __syncthreads();
        scan_pick(k0, k1);
        __syncthreads();
        hi0 = ss.cut_d[0]; k0 = ss.cut_r[0];
        if (nsets > 1) { hi1 = ss.cut_d[1]; k1 = ss.cut_r[1]; }
        __syncthreads();
        clear_hist();
        __syncthreads();
        for (int s = 0; s < nsets; s++) {
            VS_SPAN(key_t*, a, VS_SPAN_RAW(s ? a1 : a0), nt, 117);
            const uint32_t hi = s ? hi1 : hi0;
            walk_strided(a, [&](uint32_t key) {
                const uint32_t d = key >> 16;
                if ((d >> 8) == hi) bump(s, d & 255u);
            });
        }
        __syncthreads();
    }
    scan_pick(k0, k1);
    __syncthreads();
    const uint32_t D0 = (hi0 << 8) | ss.cut_d[0], R0 = ss.cut_r[0];
    const uint32_t D1 = nsets > 1 ? ((hi1 << 8) | ss.cut_d[1]) : 0u, R1 = nsets > 1 ? ss.cut_r[1] : 0u;
    // ---- placement: wave w owns tiles [w * per, (w + 1) * per) of every set (per a multiple of 64), a lane one tile of every
    // 64: the tiles before a tile, within its step, are a ballot and a masked bit count; the steps and waves before it are
    // wave-uniform running sums.  First the per-wave totals {less, equal} per set (packed into one 64-bit word, each field
    // < 65536) and one barrier, then the same walk again with the stores.
    constexpr int kNW = kGnThreads / 64, kP = 4;
    const int per = ((nt + kNW - 1) / kNW + 63) & ~63;
    const int w_lo = min(wave * per, nt), w_hi = min(w_lo + per, nt);
    auto below = [&](unsigned long long m) -> uint32_t {
        return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    };
    unsigned long long mine = 0ull;
    for (int s = 0; s < nsets; s++) {
        VS_SPAN(key_t*, a, VS_SPAN_RAW(s ? a1 : a0), nt, 117);
        const uint32_t D = s ? D1 : D0;
        uint32_t less = 0u, eq = 0u;
        for (int i0 = w_lo; i0 < w_hi; i0 += 64 * kP) {
            uint32_t v[kP];
#pragma unroll
            for (int u = 0; u < kP; u++) v[u] = a[min(i0 + 64 * u + lane, nt - 1)];
#pragma unroll
            for (int u = 0; u < kP; u++) {
                const uint32_t d = (i0 + 64 * u + lane < w_hi) ? (v[u] >> 16) : 0xffffffffu;
                less += (uint32_t)__popcll(__ballot(d < D));
                eq += (uint32_t)__popcll(__ballot(d == D));
            }
        }
        mine |= ((unsigned long long)(less | (eq << 16))) << (32 * s);
    }
    if (lane == 0) ss.wsum[wave] = mine;
    __syncthreads();
    unsigned long long before = 0ull;
    for (int w = 0; w < wave; w++) before += ss.wsum[w];
    for (int s = 0; s < nsets; s++) {
        VS_SPAN(key_t*, a, VS_SPAN_RAW(s ? a1 : a0), nt, 117);
        VS_SPAN(out_t*, o, VS_SPAN_RAW(s ? o1 : o0), nt, 118);
        const uint32_t D = s ? D1 : D0, R = s ? R1 : R0;
        uint32_t less = (uint32_t)(before >> (32 * s)) & 0xffffu, eq = (uint32_t)(before >> (32 * s + 16)) & 0xffffu;
        for (int i0 = w_lo; i0 < w_hi; i0 += 64 * kP) {
            uint32_t v[kP];
#pragma unroll
            for (int u = 0; u < kP; u++) v[u] = a[min(i0 + 64 * u + lane, nt - 1)];
#pragma unroll
            for (int u = 0; u < kP; u++) {
                const int i = i0 + 64 * u + lane;
                const uint32_t d = i < w_hi ? (v[u] >> 16) : 0xffffffffu;
                const unsigned long long ml = __ballot(d < D), me = __ballot(d == D);
                const uint32_t my_less = less + below(ml), my_eq = eq + below(me);
                if (d < D || (d == D && my_eq < R)) o[my_less + min(my_eq, R)] = (uint16_t)i;
                less += (uint32_t)__popcll(ml);
                eq += (uint32_t)__popcll(me);
            }
        }
    }
    __syncthreads();                                                         // the survivors are placed
}


// Kernel-level selection op (one block per array): out_idx[0..nsel) = tile indices in the order
// std::nth_element leaves them.  status[b] = 1 when the depth limit was hit.
__global__ VS_GN_FUSED_BOUNDS __attribute__((unused)) void vs_k_select(const uint16_t* __restrict__ wd, int nt, int nsel,
                                                          int32_t* __restrict__ out_idx, int32_t* __restrict__ status, int rule) {
    extern __shared__ __attribute__((aligned(16))) uint8_t dyn[];
    __shared__ SelShared ss;
    __shared__ StableShared sts;
    uint32_t* a = (uint32_t*)dyn;
    uint16_t* posR = (uint16_t*)(a + nt);
    wd += (size_t)blockIdx.x * nt;
    out_idx += (size_t)blockIdx.x * nt;
    for (int i = threadIdx.x; i < nt; i += kGnThreads) a[i] = ((uint32_t)wd[i] << 16) | (uint32_t)i;
    __syncthreads();
    if (rule) {          // VS_SELECT_STABLE's rule: the survivors' tile indices arrive in posR, in tile order
        stable_select<true>(a, posR, a, posR, 1, nt, nsel, sts);
        for (int i = threadIdx.x; i < nsel; i += kGnThreads) out_idx[i] = (int32_t)posR[i];
        if (status != nullptr && threadIdx.x == 0) status[blockIdx.x] = 0;
        return;
    }
    const int r = introselect_block(a, posR, ss, nt, nsel);
    for (int i = threadIdx.x; i < nsel; i += kGnThreads) out_idx[i] = (int32_t)(a[i] & 0xffffu);
    if (threadIdx.x == 0) status[blockIdx.x] = r;
}


__global__ VS_GN_FUSED_BOUNDS void vs_k_align_pairs(PairState* __restrict__ states,
                                                               const PairDesc* __restrict__ descs,
                                                               const uint8_t* __restrict__ pyr, size_t pyr_frame,
                                                               const uint16_t* __restrict__ lm_tab, size_t lm_frame,
                                                               const float* __restrict__ jac_tab, size_t jac_frame,
                                                               uint8_t* __restrict__ recs, size_t recs_pair,
                                                               int nt_cap, int dyn_bytes, FusedLevels fl, GnParams gp,
                                                               int group, uint8_t* __restrict__ coop, int epoch,
                                                               float* __restrict__ wv_all, PairDescPack dpack, int direct,
                                                               uint8_t* __restrict__ selbuf, size_t selbuf_pair) {
    extern __shared__ __attribute__((aligned(16))) uint8_t dyn[];
    __shared__ SelShared ss2[2];
    __shared__ GnShared sh;
    __shared__ int s_coop[2];
    // tail of a selection that runs on global arrays (introselect_block_g): values + rank table of the last <= 257 elements
    __shared__ __attribute__((aligned(16))) uint32_t sel_tail[(kWaveRange + 1) + (kWaveRange + 2) / 2 + 32];
    static_assert(sizeof(StableShared) <= sizeof(sel_tail), "VS_SELECT_STABLE keeps its histograms in the tail block (unused in that mode)");
    // dynamic LDS: the selection arrays (a | posR) at the start -- except at the coarsest level when its image AND its arrays
    // fit: then the image comes first and stays for the whole level (sparse_warpdiff and every Gauss-Newton pass sample it
    // from LDS), and the arrays follow it
    uint32_t* a = (uint32_t*)dyn;
    uint16_t* posR = (uint16_t*)(a + nt_cap);
    // `group` workgroups per pair: the first is the leader, the others help with the large levels (CoopCtrl, vs_engine.hip).
    // Everything that crosses between workgroups is written with sc1 stores and read with sc1 loads (relaxed agent-scope
    // atomics / the two inline-asm helpers below): they bypass the per-CU L1 and do not stay in the writer's L2, so no
    // cache write-back or invalidate is needed -- the hand-off is: stores, s_waitcnt vmcnt(0) in every storing wave,
    // workgroup barrier, one lane's flag store; the reader polls the flag, then barrier, then loads.
    // Pair of this workgroup.  Consecutive pairs share images (two pairs sample every keyframe, at the same keypoints; two
    // pairs read every other frame as their template), and workgroups go to the XCDs round-robin: a full batch gives every
    // XCD a contiguous run of pairs (workgroup b = the (b >> 3)-th pair of XCD b & 7's run), so that the second user of a
    // line finds it in that XCD's L2.
    int p = blockIdx.x / group;
    const int g = blockIdx.x % group;
    if (group == 1) {
        const int n = (int)gridDim.x, x = (int)blockIdx.x & 7;
        p = (n >> 3) * x + min(x, n & 7) + ((int)blockIdx.x >> 3);
    }
    CoopCtrl* const cc = group > 1 ? (CoopCtrl*)(coop + (size_t)p * coop_pair_bytes(nt_cap)) : nullptr;
    uint32_t* const gkeys = group > 1 ? (uint32_t*)((uint8_t*)cc + kCoopCtrlBytes) : nullptr;      // 2 * nt_cap packed keys
    // the sampled values of sparse_warpdiff, tile i of the x-set at [i], of the y-set at [nt + i]: the gather turns them into
    // the first iteration's residuals (PointRecs::r0).  Written by whoever computes the tile (helpers: sc1), always read sc1.
    // Helper workgroups hand theirs over in the exchange block (gvals, sc1 only, like the keys); the leader copies them into wv,
    // which only this workgroup touches (plain stores and loads).
    float* const wv = wv_all + (size_t)p * 2 * nt_cap;
    float* const gvals = group > 1 ? (float*)(gkeys + 2 * (size_t)nt_cap) : nullptr;
    float* const gtpx = group > 1 ? gvals + 2 * (size_t)nt_cap : nullptr;              // the template pixel of the tile, as the records hold it
    float* const wt = wv + (size_t)gridDim.x / group * 2 * nt_cap;                      // second half of the buffer: template pixels
    auto ld_sc1 = [](const int* f) { return __hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    auto st_sc1 = [](int* f, int v) { __hip_atomic_store(f, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    auto ldd_sc1 = [](const double* f) { return __hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    auto std_sc1 = [](double* f, double v) { __hip_atomic_store(f, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    // one thread polls (bounded: ~0.3 s); false = the pair ended early (helpers only) or timed out
    auto flag_wait = [&](const int* f) -> bool {
        for (int it = 0; it < (1 << 18); it++) {
            if (ld_sc1(f) == epoch) return true;
            if (g > 0 && ld_sc1(&cc->abort) == epoch) return false;
            __builtin_amdgcn_s_sleep(4);                        // (idle helpers poll for ~200 us: keep them off the fabric)
        }
        return false;
    };
    // direct: `states` is the host's pinned result block (written, never read) and the descriptors are in the arguments
    PairState& st = states[p];
    const PairDesc d = direct ? dpack.d[p] : descs[p];
    // alignment.cpp:344 identity, or the phase-correlation start value the host side put into the state (:376-387)
    double T[4] = {0.0, 0.0, 0.0, 0.0};
    if (!direct) { T[0] = st.T[0]; T[1] = st.T[1]; T[2] = st.T[2]; T[3] = st.T[3]; }
    int fail = 0, fail_level = 0;
    if (g > 0 && threadIdx.x == 0) st_sc1(&cc->arrived[g], epoch);
    for (int l = fl.levels - 1; l >= 0 && !fail; l--) {
        const int w = fl.w[l], h = fl.h[l], nt = fl.nt[l], nsel = fl.nsel[l];
        const bool share = group > 1 && nt >= kCoopMinTiles;
        if (g > 0 && !share) continue;
        int my_slice = 0, nslices = 1;
        if (g > 0) {
            // helper: wait for the leader to open the level, take the slice it handed out (none if this workgroup started late)
            if (threadIdx.x == 0) s_coop[0] = flag_wait(&cc->lv[l].t_ready) ? 1 : 0;
            __syncthreads();
            if (!s_coop[0]) return;
            // (independent loads: one trip to memory)
            const int sl_ = ld_sc1(&cc->lv[l].assign[g]), ns_ = ld_sc1(&cc->lv[l].nslices);
            const double t0_ = ldd_sc1(&cc->lv[l].T[0]), t1_ = ldd_sc1(&cc->lv[l].T[1]), t2_ = ldd_sc1(&cc->lv[l].T[2]), t3_ = ldd_sc1(&cc->lv[l].T[3]);
            my_slice = sl_; nslices = ns_;
            T[0] = t0_; T[1] = t1_; T[2] = t2_; T[3] = t3_;
            __syncthreads();               // s_coop is reused at the next level
            if (my_slice < 0) continue;
        }
        const uint8_t* tmpl = pyr + (size_t)d.tmpl_slot * pyr_frame + fl.img_off[l];
        const uint8_t* key = pyr + (size_t)d.key_slot * pyr_frame + fl.img_off[l];
        const PointRecs rc = pair_recs(recs, recs_pair, p, nt_cap);
        float P[4];
        ul_params_sparse(T, w, h, P);
        const float A1 = 1.0f + P[0];
        const uint16_t* lm0 = lm_tab + (size_t)d.key_slot * lm_frame + fl.lm_off[l];
        const float* jac0 = jac_tab + (size_t)d.key_slot * jac_frame + fl.jac_off[l];
        // The coarsest level's image is copied into the dynamic LDS block when it fits: most of a pair's Gauss-Newton iterations
        // happen there and then gather from LDS.  (Finer levels usually run a single iteration, which does not repay the
        // copy: measured.)  Before sparse_warpdiff when the selection arrays fit behind it, else after the selection.
        auto stage_image = [&]() {
            const uint32_t* src = (const uint32_t*)key;          // level images start on 256-byte boundaries
            uint32_t* dst = (uint32_t*)dyn;
            typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
            const VS_GLOBAL_AS u32x4* __restrict__ s4 = (const VS_GLOBAL_AS u32x4*)key;
            VS_LDS_AS u32x4* __restrict__ d4 = (VS_LDS_AS u32x4*)(uintptr_t)(unsigned)(uintptr_t)dyn;
            const int n4 = (w * h) / 16;                         // 16 bytes per load, four loads in flight per thread
            for (int i = threadIdx.x; i < n4; i += 4 * kGnThreads) {
                u32x4 v[4];
#pragma unroll
                for (int u = 0; u < 4; u++) v[u] = s4[min(i + u * kGnThreads, n4 - 1)];
#pragma unroll
                for (int u = 0; u < 4; u++) if (i + u * kGnThreads < n4) d4[i + u * kGnThreads] = v[u];
            }
            for (int i = n4 * 4 + threadIdx.x; i < (w * h) / 4; i += kGnThreads) dst[i] = src[i];
            VS_BOUNDS_CHECK((w * h) / 4 + 1, dyn_bytes / 4, 120);        // the staged image + its pad lie inside the dynamic block
            if (threadIdx.x < 2) dst[(w * h) / 4 + threadIdx.x] = 0u;    // the pad read by the aligned-pair loads
        };
        const int img_bytes = (w * h + 8 + 15) & ~15;
        const bool img_fits = l == fl.levels - 1 && w * h + 8 <= dyn_bytes && (w * h & 3) == 0;
        const bool img_first = img_fits && g == 0 && img_bytes + 12 * nt <= dyn_bytes && nt <= 32 * (kGnThreads / 2);
        // a level whose selection arrays (6 B per tile, one point set at a time) do not fit the dynamic LDS block selects on the
        // pair's global scratch instead (the small-footprint build at a 4K level 0)
        const bool sel_global = selbuf != nullptr && 6 * nt > dyn_bytes;
        if (img_first) {
            stage_image();
            a = (uint32_t*)(dyn + img_bytes);
            __syncthreads();
        } else if (sel_global) {
            a = (uint32_t*)(selbuf + (size_t)p * selbuf_pair);
            posR = (uint16_t*)(a + nt_cap);
        } else {
            a = (uint32_t*)dyn;
            if (selbuf != nullptr) posR = (uint16_t*)(a + nt);     // (the small build's LDS block is sized per level, not for nt_cap)
        }
        const vs_lbytes lkey_img = (vs_lbytes)(uintptr_t)(unsigned)(uintptr_t)dyn;
        // sparse_warpdiff (generators.cpp:646-700) of the tile keypoints, packed for the selection: dst[i] = diff << 16 | tile.
        // One workgroup owns the pair, so nothing but the thread's own independent loads hides the memory latency: each
        // thread keeps kWdFlight points in flight (their four row gathers + the template pixel are issued before the first
        // result is computed) and fetches the next group's keypoint coordinates while the current group computes.
        // `both`: the x-set and the y-set back to back (index i >= nt is tile i - nt of the y-set, whose coordinates start
        // 2*nt further on); otherwise `count` tiles of the one set that starts at lmb.
        // Order of the points when both sets are walked together: tile row by tile row, the x-set tiles of a row and then its
        // y-set tiles.  The two keypoints of a tile lie within one tile of each other, so the second set finds most of its
        // 128-byte lines still in L1 / L2 (set after set, every line is fetched twice: with hundreds of pairs in flight the
        // pass is bound by exactly that traffic).  Point i -> set, tile t; keys / samples are stored at [set * nt + t].
        const int row_pts = 2 * fl.tx[l];
        auto point_tile = [&](int i, int& set, int& t) {
            const int j = i / row_pts, q = i - j * row_pts;
            set = q >= fl.tx[l] ? 1 : 0;
            t = j * fl.tx[l] + q - set * fl.tx[l];
        };
        constexpr int kWdFlight = 1;      // (4 and 2 measured 2-4 % slower, alone and in a full batch: the pass is bound by line fetches, and fewer
                                          // points in flight keep the rows a workgroup touches at a time inside its share of the L2)
        auto warpdiff_fill = [&](auto gkey, uint32_t* dst, const uint16_t* __restrict__ lmb, int count, bool both, int voff) {   // values to wv[voff + i]
            const vs_gbytes gtmpl = (vs_gbytes)tmpl;
            const VS_GLOBAL_AS uint32_t* __restrict__ gxy = (const VS_GLOBAL_AS uint32_t*)lmb;
            uint32_t lx[kWdFlight], ly[kWdFlight];
            auto load_lm = [&](int b) {
#pragma unroll
                for (int u = 0; u < kWdFlight; u++) {
                    const int i = min(b + u * kGnThreads, count - 1);
                    int set = 0, t = i;
                    if (both) point_tile(i, set, t);
                    const uint32_t xy = gxy[set * nt + t];     // the tile's {x, y} pair
                    lx[u] = xy & 0xffffu; ly[u] = xy >> 16;
                }
            };
            int base = threadIdx.x;
            if (base < count) load_lm(base);
            while (base < count) {
                LanczosFetch f[kWdFlight];
                uint32_t tp[kWdFlight];
#pragma unroll
                for (int u = 0; u < kWdFlight; u++) {
                    const int tile_x = min((int)lx[u], w - 1), tile_y = min((int)ly[u], h - 1);
                    const float ox = (float)tile_x, oy = (float)tile_y;
                    const float Wx = A1 * ox - P[1] * oy + P[2];
                    const float Wy = P[1] * ox + A1 * oy + P[3];
                    f[u] = lanczos_fetch(gkey, w, h, w, Wx, Wy);
                    tp[u] = gtmpl[(size_t)tile_y * w + tile_x];
                }
                const int nb = base + kWdFlight * kGnThreads;
                if (nb < count) load_lm(nb);
#pragma unroll
                for (int u = 0; u < kWdFlight; u++) {
                    const int i = base + u * kGnThreads;
                    const float v = lanczos_finish(f[u], w);
                    float diff = fabsf(v - (float)tp[u]);
                    diff = fminf(fmaxf(diff, 0.0f), 65535.0f);
                    if (i < count) {
                        int set = 0, t = i;
                        if (both) point_tile(i, set, t);
                        const int o = set * nt + t;
                        VS_BOUNDS_CHECK(o, both ? 2 * nt : nt, 121);
                        VS_BOUNDS_CHECK(voff + o, 2 * nt_cap, 122);
                        dst[o] = ((uint32_t)(uint16_t)diff << 16) | (uint32_t)t;
                        wv[voff + o] = v;
                        wt[voff + o] = (float)tp[u];
                    }
                }
                base = nb;
            }
        };
        // The same for a slice [i0, i1) of both sets (helper-workgroup levels), keys to device memory.  A slice is short
        // (a few points per thread) and everything it touches is cold in this CU's caches, so the point is to have all of a
        // thread's loads in flight at once: coordinates of up to four points, then their gathers, then the arithmetic.  The
        // keys are staged in LDS (`stage`, free at this time) and leave with 16-byte sc1 stores (i0 and the buffer are
        // 16-byte aligned).
        auto warpdiff_slice = [&](uint32_t* __restrict__ dst, uint32_t* stage, int i0_all, int i1_all) {
            const vs_gbytes gkey = (vs_gbytes)key, gtmpl = (vs_gbytes)tmpl;
            const VS_GLOBAL_AS uint32_t* __restrict__ gxy = (const VS_GLOBAL_AS uint32_t*)lm0;
            lds_u32* __restrict__ stg = (lds_u32*)stage;
            const int cap = (dyn_bytes / 12) & ~63;              // points per pass: key, value and template pixel staged, 12 bytes
            for (int i0 = i0_all; i0 < i1_all; i0 += cap) {
            const int i1 = min(i0 + cap, i1_all), n = i1 - i0;
            for (int base = threadIdx.x; base < n; base += 4 * kGnThreads) {
                uint32_t lx[4], ly[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int i = i0 + min(base + u * kGnThreads, n - 1);
                    const uint32_t xy = gxy[i];                  // pairs of the x-set, then of the y-set: index = storage index
                    lx[u] = xy & 0xffffu; ly[u] = xy >> 16;
                }
                LanczosFetch f[4];
                uint32_t tp[4];
                float vv[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int tile_x = min((int)lx[u], w - 1), tile_y = min((int)ly[u], h - 1);
                    const float ox = (float)tile_x, oy = (float)tile_y;
                    f[u] = lanczos_fetch(gkey, w, h, w, A1 * ox - P[1] * oy + P[2], P[1] * ox + A1 * oy + P[3]);
                    tp[u] = gtmpl[(size_t)tile_y * w + tile_x];
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int q = base + u * kGnThreads, i = i0 + q;
                    vv[u] = lanczos_finish(f[u], w);
                    float diff = fabsf(vv[u] - (float)tp[u]);
                    diff = fminf(fmaxf(diff, 0.0f), 65535.0f);
                    if (q < n) {
                        VS_BOUNDS_CHECK(2 * n + q, dyn_bytes / 4, 123);   // key | value | template pixel, n of each, in the dynamic block
                        stg[q] = ((uint32_t)(uint16_t)diff << 16) | (uint32_t)(i - (i >= nt ? nt : 0));
                        stg[n + q] = __float_as_uint(vv[u]);
                        stg[2 * n + q] = __float_as_uint((float)tp[u]);
                    }
                }
            }
            __syncthreads();
            typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
            for (int q = 4 * (int)threadIdx.x; q < n; q += 4 * kGnThreads) {
                if (q + 4 <= n) {
                    // (s_nop: a store of more than 8 bytes reads its data registers late; the compiler pads real instructions
                    // against an overwrite by the next VALU instruction but cannot see into inline asm)
                    const u32x4 v = {stg[q], stg[q + 1], stg[q + 2], stg[q + 3]}, x = {stg[n + q], stg[n + q + 1], stg[n + q + 2], stg[n + q + 3]},
                                y = {stg[2 * n + q], stg[2 * n + q + 1], stg[2 * n + q + 2], stg[2 * n + q + 3]};
                    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" :: "v"(dst + i0 + q), "v"(v) : "memory");
                    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" :: "v"(gvals + i0 + q), "v"(x) : "memory");
                    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" :: "v"(gtpx + i0 + q), "v"(y) : "memory");
                } else {
                    for (int u = 0; q + u < n; u++) {
                        st_sc1((int*)dst + i0 + q + u, (int)stg[q + u]); st_sc1((int*)gvals + i0 + q + u, (int)stg[n + q + u]);
                        st_sc1((int*)gtpx + i0 + q + u, (int)stg[2 * n + q + u]);
                    }
                }
            }
            __syncthreads();                                     // the stage is refilled by the next pass
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // every storing wave, before the barrier that precedes the flag
        };
        // gather (alignment.cpp:523-546) in the order nth_element left the survivors: record `slot0 + j` = tile sel[j] & 0xffff
        // of the set at lmb / jacb, kGaFlight records in flight per thread.  The Hessian of the level (alignment.cpp:278-332,
        // upper triangle of sum j j^T in fp64) is accumulated on the way: thread t sums records t, t + kGnThreads, ... in
        // that order, exactly as gn_hessian_partials does over the finished records (the per-level kernel of the host-selection
        // path), so H is the same bit for bit without the second pass.
        constexpr int kGaFlight = 4;
        double hacc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        double fa8[8] = {0, 0, 0, 0, 0, 0, 0, 0};      // the first Gauss-Newton pass, from the residuals as they are written
        auto gather_fill = [&](const uint32_t* sel, const uint16_t* sel16, int count, bool both, const uint16_t* __restrict__ lmb,
                               const float* __restrict__ jacb, int slot0, int voff) {
            // (VS_SELECT_STABLE hands the survivors over as 16-bit tile indices, sel16, laid out like sel: the y-set's nt further on)
            const lds_u16* __restrict__ lsel16 = (const lds_u16*)sel16;
            const VS_GLOBAL_AS uint16_t* __restrict__ gsel16 = (const VS_GLOBAL_AS uint16_t*)sel16;
            typedef float f32x4g __attribute__((ext_vector_type(4)));
            const VS_GLOBAL_AS uint32_t* __restrict__ gxy = (const VS_GLOBAL_AS uint32_t*)lmb;
            const VS_GLOBAL_AS f32x4g* __restrict__ gj = (const VS_GLOBAL_AS f32x4g*)jacb;
            const lds_u32* __restrict__ lsel = (const lds_u32*)sel;
            const glb_u32* __restrict__ gsel = (const glb_u32*)sel;       // (the selection ran on the pair's global scratch: sel_global)
            // thread t takes the records whose slot is t modulo kGnThreads (slot0 is not a multiple of it for the second set
            // of the set-by-set path)
            int first = (int)threadIdx.x - slot0 % kGnThreads;
            if (first < 0) first += kGnThreads;
            for (int base = first; base < count; base += kGaFlight * kGnThreads) {
                uint32_t px[kGaFlight], py[kGaFlight];
                float jv[kGaFlight][4], sv[kGaFlight], tp[kGaFlight];
#pragma unroll
                for (int u = 0; u < kGaFlight; u++) {
                    const int j = min(base + u * kGnThreads, count - 1);
                    // both: survivors of the x-set at sel[0, nsel), of the y-set at sel[nt, nt + nsel)
                    const int set = (both && j >= nsel) ? 1 : 0;
                    VS_BOUNDS_CHECK(j + set * (nt - nsel), both ? 2 * nt : nt, 124);
                    const int t = sel16 != nullptr ? (int)(sel_global ? gsel16[j + set * (nt - nsel)] : lsel16[j + set * (nt - nsel)])
                                                   : (int)((sel_global ? gsel[j + set * (nt - nsel)] : lsel[j + set * (nt - nsel)]) & 0xffffu);
                    VS_BOUNDS_CHECK(t, nt, 125);                        // a survivor is a tile of the level
                    VS_BOUNDS_CHECK(voff + set * nt + t, 2 * nt_cap, 126);
                    const uint32_t xy = gxy[set * nt + VS_DEBUG_CLAMP(t, nt)];
                    px[u] = xy & 0xffffu; py[u] = xy >> 16;
                    const f32x4g jq = gj[set * nt + VS_DEBUG_CLAMP(t, nt)];
                    jv[u][0] = jq.x; jv[u][1] = jq.y; jv[u][2] = jq.z; jv[u][3] = jq.w;
                    sv[u] = wv[voff + set * nt + t];
                    tp[u] = wt[voff + set * nt + t];     // = float(template pixel at the clamped keypoint), kept by sparse_warpdiff
                }
#pragma unroll
                for (int u = 0; u < kGaFlight; u++) {
                    const int j = base + u * kGnThreads;
                    if (j < count) {
                        const int slot = slot0 + j;
                        VS_BOUNDS_CHECK(slot, 2 * nt_cap, 127);
                        rc.xy[slot] = px[u] | (py[u] << 16);
                        rc.tv[slot] = tp[u];
                        const float r0 = tp[u] - sv[u];
                        rc.r0[slot] = r0;
                        rc.j[slot] = make_float4(jv[u][0], jv[u][1], jv[u][2], jv[u][3]);
                        if (kVF == 1) {     // (a build with virtual threads sums over the finished records instead: gn_hessian_partials)
                            first_pass_terms(slot, nsel, jv[u], r0, fa8);
                            const double jd[4] = {(double)jv[u][0], (double)jv[u][1], (double)jv[u][2], (double)jv[u][3]};
                            int k = 0;
#pragma unroll
                            for (int a2 = 0; a2 < 4; a2++)
#pragma unroll
                                for (int b2 = a2; b2 < 4; b2++) hacc[k++] += jd[a2] * jd[b2];
                        }
                    }
                }
            }
        };
        const bool dual = (img_first ? img_bytes : 0) + 12 * nt <= dyn_bytes && nt <= 32 * (kGnThreads / 2);
        if (g > 0) {
            // helper: sparse_warpdiff of my slice, then tell the leader
            const int sl = ((2 * nt + nslices - 1) / nslices + 63) & ~63;
            warpdiff_slice(gkeys, a, my_slice * sl, min((my_slice + 1) * sl, 2 * nt));
            __syncthreads();
            if (threadIdx.x == 0 && !gp.stall_helpers) st_sc1(&cc->lv[l].wd_done[g], epoch);
            continue;
        }
        if (share) {
            // leader: hand slices to the helpers that have arrived by now; never wait for one that has not
            if (threadIdx.x < 64) {        // lane gg looks at helper gg: one trip to memory for all of them
                const int gg = threadIdx.x;
                const bool cand = gg >= 1 && gg < group;
                const bool here = cand && ld_sc1(&cc->arrived[gg]) == epoch;
                const unsigned long long m = __ballot(here);
                if (cand) st_sc1(&cc->lv[l].assign[gg], here ? 1 + __popcll(m & ((1ull << gg) - 1)) : -1);
                if (gg == 0) {
                    st_sc1(&cc->lv[l].nslices, 1 + __popcll(m));
                    std_sc1(&cc->lv[l].T[0], T[0]); std_sc1(&cc->lv[l].T[1], T[1]); std_sc1(&cc->lv[l].T[2], T[2]); std_sc1(&cc->lv[l].T[3], T[3]);
                }
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                if (gg == 0) {
                    st_sc1(&cc->lv[l].t_ready, epoch);
                    s_coop[0] = 1 + __popcll(m);
                    s_coop[1] = (int)(unsigned)m;              // who takes part (group <= 16)
                }
            }
            __syncthreads();
            nslices = s_coop[0];
        }
        const bool shared_now = share && nslices > 1;
        if (shared_now) {
            // my own slice (slice 0), then wait for the helpers that took one; then the keys are read back into LDS below
            const int sl = ((2 * nt + nslices - 1) / nslices + 63) & ~63;
            warpdiff_slice(gkeys, a, 0, min(sl, 2 * nt));
            __syncthreads();
            const unsigned part = (unsigned)s_coop[1];
            __syncthreads();
            if (threadIdx.x < 64) {        // lane gg polls helper gg
                const int gg = threadIdx.x;
                bool done = gg >= group || !((part >> (gg & 31)) & 1u);
                int ok = 0;
                for (int it = 0; it < (1 << 18); it++) {
                    if (!done) done = ld_sc1(&cc->lv[l].wd_done[gg & 15]) == epoch;
                    if (__all(done)) { ok = 1; break; }
                    __builtin_amdgcn_s_sleep(1);
                }
                if (gg == 0) s_coop[1] = ok;
            }
            __syncthreads();
            if (!s_coop[1]) { fail = 101; fail_level = l; }       // a helper timed out: the host redoes the pair
        }
        // words [k0, k0 + n) of an exchange array (keys -> LDS, sampled values -> wv): 16-byte sc1 loads, four in flight per thread
        auto read_exchange = [&](const uint32_t* from, uint32_t* dst_lds, int k0, int n) {
            typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
            const uint32_t* src = from + k0;
            const int nv = n >> 2;
            for (int q = threadIdx.x; q < nv; q += 4 * kGnThreads) {
                u32x4 v[4];
                const uint32_t* p0 = src + 4 * (size_t)min(q, nv - 1);
                const uint32_t* p1 = src + 4 * (size_t)min(q + kGnThreads, nv - 1);
                const uint32_t* p2 = src + 4 * (size_t)min(q + 2 * kGnThreads, nv - 1);
                const uint32_t* p3 = src + 4 * (size_t)min(q + 3 * kGnThreads, nv - 1);
                asm volatile("global_load_dwordx4 %0, %4, off sc1\n\tglobal_load_dwordx4 %1, %5, off sc1\n\t"
                             "global_load_dwordx4 %2, %6, off sc1\n\tglobal_load_dwordx4 %3, %7, off sc1\n\ts_waitcnt vmcnt(0)"
                             : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]) : "v"(p0), "v"(p1), "v"(p2), "v"(p3) : "memory");
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int qq = q + u * kGnThreads;
                    VS_BOUNDS_CHECK(4 * min(qq, nv - 1) + 3, n, 128);
                    if (qq < nv) { dst_lds[4 * qq] = v[u].x; dst_lds[4 * qq + 1] = v[u].y; dst_lds[4 * qq + 2] = v[u].z; dst_lds[4 * qq + 3] = v[u].w; }
                }
            }
            for (int i = (nv << 2) + threadIdx.x; i < n; i += kGnThreads) dst_lds[i] = (uint32_t)ld_sc1((const int*)src + i);
        };
        if (fail) {
        } else if (dual) {
            // both sets side by side: aX | aY | posRX | posRY inside the same dynamic LDS block
            uint32_t* aX = a;
            uint32_t* aY = a + nt;
            uint16_t* pRX = (uint16_t*)(a + 2 * nt);
            uint16_t* pRY = pRX + nt;
            if (shared_now) { read_exchange(gkeys, a, 0, 2 * nt); read_exchange((const uint32_t*)gvals, (uint32_t*)wv, 0, 2 * nt); read_exchange((const uint32_t*)gtpx, (uint32_t*)wt, 0, 2 * nt); }
            else if (img_first) warpdiff_fill(lkey_img, a, lm0, 2 * nt, true, 0);
            else warpdiff_fill((vs_gbytes)key, a, lm0, 2 * nt, true, 0);
            __syncthreads();
            if (gp.sel_stable) stable_select<true>(aX, pRX, aY, pRY, 2, nt, nsel, *reinterpret_cast<StableShared*>(sel_tail));
            else if (introselect_dual(aX, pRX, aY, pRY, ss2, nt, nsel, gp.sel_depth_cap)) { fail = 100; fail_level = l; }
            gather_fill(a, gp.sel_stable ? pRX : nullptr, 2 * nsel, true, lm0, jac0, 0, 0);
        } else {
            for (int set = 0; set < 2 && !fail; set++) {
                const uint16_t* lm = lm0 + (size_t)set * 2 * nt;
                const float* jac = jac0 + (size_t)set * 4 * nt;
                if (shared_now) {
                    read_exchange(gkeys, a, set * nt, nt); read_exchange((const uint32_t*)gvals, (uint32_t*)wv + set * nt, set * nt, nt);
                    read_exchange((const uint32_t*)gtpx, (uint32_t*)wt + set * nt, set * nt, nt);
                } else warpdiff_fill((vs_gbytes)key, a, lm, nt, false, set * nt);
                __syncthreads();
                if (gp.sel_stable) {
                    if (sel_global) stable_select<false>(a, posR, a, posR, 1, nt, nsel, *reinterpret_cast<StableShared*>(sel_tail), dyn, dyn_bytes);
                    else stable_select<true>(a, posR, a, posR, 1, nt, nsel, *reinterpret_cast<StableShared*>(sel_tail));
                } else if (sel_global ? introselect_block_g(a, posR, ss2[0], sel_tail, nt, nsel, gp.sel_depth_cap)
                                    : introselect_block(a, posR, ss2[0], nt, nsel, gp.sel_depth_cap)) { fail = 100; fail_level = l; }
                gather_fill(a, gp.sel_stable ? posR : nullptr, nsel, false, lm, jac, set * nsel, set * nt);
                __syncthreads();   // a[] is refilled by the next set
            }
        }
        if (kVF == 1) {
            wave_partials<10>(hacc, sh.red[0]);
            wave_partials8_butterfly(fa8, sh.red[1], (int)threadIdx.x >> 6);
        } else {
            // virtual threads: the records are complete behind this barrier; every hardware thread then adds the records of the
            // virtual threads it stands for, in the order the full-size build adds them while it writes them
            __syncthreads();
            if (!fail) gn_hessian_partials(sh, rc, nsel);
        }
        __syncthreads();           // the record stores, the Hessian partials and the first pass's sums are visible block-wide
        if (fail) break;
        const uint8_t* key_lds = nullptr;
        if (img_fits) {
            if (!img_first) { stage_image(); __syncthreads(); }   // (the selection arrays in the block are dead now)
            key_lds = dyn;
        }
        int iters;
        double cond;
        const int f = gn_level(sh, key, key_lds, w, h, nsel, rc, l, gp, T, &iters, &cond);
        if (threadIdx.x == 0) {
            st.iterations[l] = iters; st.condition[l] = cond;
            if (f != 2) {    // the estimate the level ended on, before gn_level's x2 of TX,TY (halving undoes it exactly)
                const double u = (!f && l > 0) ? 0.5 : 1.0;
                st.level_T[l][0] = T[0]; st.level_T[l][1] = T[1]; st.level_T[l][2] = T[2] * u; st.level_T[l][3] = T[3] * u;
            }
        }
        if (f) { fail = f; fail_level = l; }
        __syncthreads();
    }
    if (g > 0) return;
    if (group > 1 && threadIdx.x == 0) st_sc1(&cc->abort, epoch);     // helpers still waiting for a level that will not come
    if (threadIdx.x == 0) {
        st.status = fail ? 0 : 1;
        st.fail_reason = fail;
        st.fail_level = fail_level;
        st.T[0] = T[0]; st.T[1] = T[1]; st.T[2] = T[2]; st.T[3] = T[3];
        if (direct) {       // the host may be polling this word in pinned memory: everything above first
            __threadfence_system();
            __hip_atomic_store(&st.pad, epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

