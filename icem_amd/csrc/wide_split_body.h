// wide_split_body.h -- the BODY of rollout_wide_split_kernel (k_rollout_wide_split.hip), included textually into the kernel that
// takes its argument block by value and into rollout_wide_split_batch_kernel (k_rollout_wide_split_batch.hip), which builds `a`
// from an array in device memory (icem_plan_step_batch): one text, and the by-value kernel compiles exactly as it did before the
// batched form existed (through a shared device function 42 of its 48 instantiations changed their instruction count, 15 their
// register count, c3's among them -- EXPERIMENTS R9.1).  Expects: template parameters NCT, KIND, EXT, FIVE, F16 and `a` (WideRolloutArgs) in scope.
// No include guard.
    constexpr int NPL = F16 ? 2 : 3;
    extern __shared__ __attribute__((aligned(16))) float X[];  // [16 * SPLIT_TT][XS] f32 rows, then the planes' buffers
    __shared__ CostArgs<float> cs_s;
    __shared__ float rscale[F16 ? 16 * SPLIT_TT : 1], rinv[F16 ? 16 * SPLIT_TT : 1];   // fp16 planes: the rows' powers of two
    __shared__ __attribute__((aligned(16))) float ksc_s[F16 ? SPLIT_KMAX : 4];       // ... the contraction entries' ...
    __shared__ __attribute__((aligned(16))) float csc_s[F16 ? 16 * SPLIT_WAVES * NCT : 4];   // ... and the output columns' (pack_wide_model_split)
    if (F16) {   // (split_batch opens with a barrier)
        for (int e = threadIdx.x; e < 32 * a.kb; e += 64 * SPLIT_WAVES) ksc_s[e] = a.ksc[e];
        for (int e = threadIdx.x; e < 16 * SPLIT_WAVES * NCT; e += 64 * SPLIT_WAVES) csc_s[e] = a.csc[e];
    }
    unsigned char* P = reinterpret_cast<unsigned char*>(X + (size_t)16 * SPLIT_TT * a.xs);   // SPLIT_PLANE_BYTES
    // (the workgroup's candidate-list scratch lies over the planes: used behind the last batch only)
    auto wg_keys = reinterpret_cast<unsigned long long(*)[SPLIT_WAVES][32]>(P);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (EXT) wide_stage_terms(cs_s, a.cs, tid, 64 * SPLIT_WAVES);
    // this wave's share of the model: [kb][wave][ct][plane][lane] 16-byte vectors
    typedef const __attribute__((address_space(1))) u32x4* gvec;
    gvec Mw = (gvec)a.Mp + (size_t)wave * NCT * NPL * 64 + lane;
    const size_t kb_stride = (size_t)SPLIT_WAVES * NCT * NPL * 64;
    auto request1 = [&](int kb, int e) -> u32x4 { return Mw[(size_t)kb * kb_stride + (size_t)e * 64]; };
    auto request = [&](u32x4 (&m)[NCT * NPL], int kb) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int e = 0; e < NCT * NPL; ++e) m[e] = request1(kb, e);
        __builtin_amdgcn_sched_barrier(0);
    };
    // tiles of this workgroup: T tiles over the grid, the remainder one each to the first workgroups
    const int tiles = (a.n_rows + 15) / 16;
    const int base = tiles / (int)gridDim.x, extra = tiles % (int)gridDim.x;
    int t_begin = (int)blockIdx.x * base + ((int)blockIdx.x < extra ? (int)blockIdx.x : extra);
    int cnt = base + ((int)blockIdx.x < extra ? 1 : 0);
    unsigned long long run_key = KEY_SENTINEL;
    bool first = true;
    u32x4 m0[NCT * NPL], m1[NCT * NPL];
    request(m0, 0);
    while (cnt > 0) {   // batches of four tiles; a remainder of five is one batch
        int ntt = cnt < SPLIT_TT - 1 ? cnt : SPLIT_TT - 1;
        if constexpr (FIVE) {
            if (cnt == SPLIT_TT) ntt = SPLIT_TT;
        }
        if constexpr (FIVE) {
            if (ntt == SPLIT_TT)
                split_batch<NCT, SPLIT_TT, KIND, EXT, true, F16>(a, X, P, rscale, rinv, ksc_s, csc_s, cs_s, t_begin * 16, ntt, tid, lane, wave, m0, m1, request1, run_key, first);
            else
                split_batch<NCT, SPLIT_TT - 1, KIND, EXT, true, F16>(a, X, P, rscale, rinv, ksc_s, csc_s, cs_s, t_begin * 16, ntt, tid, lane, wave, m0, m1, request1, run_key, first);
        } else {
            split_batch<NCT, SPLIT_TT - 1, KIND, EXT, false, F16>(a, X, P, rscale, rinv, ksc_s, csc_s, cs_s, t_begin * 16, ntt, tid, lane, wave, m0, m1, request1, run_key, first);
        }
        cnt -= ntt;
        t_begin += ntt;
    }
    __syncthreads();   // (the planes are dead: their LDS becomes the list scratch)
    if (a.K > 0) {
        FastRolloutArgs fr{};  // wg_merge_emit only looks at the candidate outputs
        fr.part_k = a.part_k;
        fr.part_c = a.part_c;
        fr.part_i = a.part_i;
        wg_merge_emit<SPLIT_WAVES>(wg_keys, run_key, a.K, lane, wave, fr);
    }
