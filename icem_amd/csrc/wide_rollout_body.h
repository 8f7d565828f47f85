// wide_rollout_body.h -- the BODY of rollout_wide_kernel (k_rollout_wide.hip: what it computes and why it is scheduled the way it is),
// included textually into the kernel that takes its argument block by value and into rollout_wide_batch_kernel
// (k_rollout_wide_batch.hip), which builds `a` from an array in device memory (icem_plan_step_batch): one text, and the by-value
// kernel compiles exactly as it did before the batched form existed (as a shared device function the same text changed the
// instruction count of 17 of the 18 by-value instantiations and the scalar spills of five; the model loop is scheduled to the
// register -- EXPERIMENTS R9.1).  Expects: template parameters NT, KIND, WAVES, EXT and `a` (WideRolloutArgs) in scope.  No include guard.
    extern __shared__ __attribute__((aligned(16))) float xs_all[];  // [WAVES][16][XS]
    __shared__ unsigned long long wg_keys[2][WAVES][32];
    constexpr int NQ = NT / 4;  // 16-byte model loads per contraction block
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int j = lane & 15, g = lane >> 4;
    const int XS = a.xs, KB = a.kb, o = a.o, d = a.d, H = a.h;
    float* X = xs_all + (size_t)wave * 16 * XS;
    const float4* __restrict__ Mp = reinterpret_cast<const float4*>(a.Mp);
    const WideCost wc{a.lin_idx, a.flip_idx, a.ctrl_w, a.lin_w, a.flip_pen, a.flip_th};
    __shared__ CostArgs<float> cs_s;
    __shared__ float park[WAVES][32];
    constexpr bool ext = EXT;
    if (EXT) wide_stage_terms(cs_s, a.cs, threadIdx.x, 64 * WAVES);
    unsigned long long run_key = KEY_SENTINEL;
    bool first = true;
    const int tiles = (a.n_rows + 15) / 16;
    for (int tile = wave * gridDim.x + blockIdx.x; tile < tiles; tile += WAVES * gridDim.x) {
        const int row0 = tile * 16;
        // contraction vectors: the start observation in every row, zeros behind
        for (int e = lane; e < 16 * XS; e += 64) {
            const int c = e % XS;
            X[e] = c < o ? a.obs0[c] : 0.f;
        }
        float acc_c = 0.f;
        // Narrow observations (NT <= 8: a step is a few hundred cycles): the NEXT step's actions are requested while this step
        // runs and held in registers -- a load -> LDS store per step would expose a global round trip that outweighs the step.
        // (At NT = 24 a step is 40 us and the kernel has no register to spare: EXPERIMENTS.md R3.12.)
        constexpr int AE = NT <= 8 ? 4 : 0;   // elements per lane held ahead: d <= 16
        const bool ahead = AE > 0 && 16 * d <= 64 * AE;
        float an[AE > 0 ? AE : 1];
        int aoff[AE > 0 ? AE : 1], xoff[AE > 0 ? AE : 1];
        if (ahead) {
#pragma unroll
            for (int i = 0; i < AE; ++i) {
                const int e = lane + 64 * i;
                const int r = e / d, c = e - r * d;
                const bool in = e < 16 * d;
                xoff[i] = in ? r * XS + o + c : -1;
                aoff[i] = (in && row0 + r < a.n_rows) ? (r * H) * d + c : -1;
            }
        }
        const float* abase = a.actions + (size_t)row0 * H * d;
        auto request_actions = [&](int t) {
#pragma unroll
            for (int i = 0; i < AE; ++i) an[i] = aoff[i] >= 0 ? abase[aoff[i] + t * d] : 0.f;
        };
        if (ahead) request_actions(0);
        for (int t = 0; t < H; ++t) {
            // this step's actions -> X[:, o .. o + d)
            if (ahead) {
#pragma unroll
                for (int i = 0; i < AE; ++i)
                    if (xoff[i] >= 0) X[xoff[i]] = an[i];
                if (t + 1 < H) request_actions(t + 1);
            } else {
                for (int e = lane; e < 16 * d; e += 64) {
                    const int r = e / d, c = e - r * d;
                    const int row = row0 + r;
                    X[r * XS + o + c] = row < a.n_rows ? a.actions[((size_t)row * H + t) * d + c] : 0.f;
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // step cost of trajectory `lane` (lanes 0..15) from the pre-action observation; with cost terms that need the
            // whole row (finite check / state box) lane (j, g) sweeps entries g, g + 4, .. of row j first
            bool bad = false;
            if (ext && cs_s.health_idx >= 0) {
                const float* xj = X + j * XS;
                bool b = false;
                for (int k = g; k < o; k += 4) b |= wide_bad_entry(cs_s, xj[k], k);
                const unsigned long long m = __ballot(b);
                bad = ((m >> (lane & 15)) & 0x0001000100010001ull) != 0ull;
            }
            // (nothing of the cost may stay in registers across the model loop below: two more live values and the
            // register allocator moves an in-flight model operand, i.e. waits for ALL requests -- 9 % of a launch.  With a
            // difference term the step's partial cost and obs[diff_idx] are parked in LDS instead.)
            const bool diff = ext && cs_s.diff_idx >= 0;
            {
                float c_step = 0.f, dold = 0.f;
                if (ext && NT <= 8) {   // narrow widths: the step is short, the term list walked by one lane is not
                    c_step = reduce_groups(wide_step_cost_lanes(wc, cs_s, X + j * XS, o, d, bad, g, dold));
                } else if (lane < 16) {
                    c_step = wide_step_cost(wc, ext, cs_s, X + lane * XS, o, d, bad, dold);
                }
                if (diff) {
                    if (lane < 16) { park[wave][lane] = c_step; park[wave][16 + lane] = dold; }
                } else {
                    acc_c = wide_accumulate(acc_c, c_step, t, a.cost_mode);
                }
            }
            f32x4 acc[NT];
#pragma unroll
            for (int ct = 0; ct < NT; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
            const float* xb = X + j * XS + g;
            // model blocks are requested ahead of the MFMAs that consume them: named register sets, the loop unrolled,
            // and scheduling barriers so that the requests stay where they are written (left alone the compiler sinks
            // them next to their first use and every block pays an L2 round trip: 2.19 instead of 1.70 ms per launch)
            float4 mA[NQ], mB[NQ], mC[NQ];
            float bA, bB, bC;
            auto request = [&](float4 (&m)[NQ], float& b, int kb) {
                kb = kb < KB ? kb : KB - 1;
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int q = 0; q < NQ; ++q) m[q] = Mp[((size_t)kb * NQ + q) * 64 + lane];
                b = xb[4 * kb];
                __builtin_amdgcn_sched_barrier(0);
            };
            auto block = [&](const float4 (&m)[NQ], float b) {
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    acc[4 * q + 0] = __builtin_amdgcn_mfma_f32_16x16x4f32(m[q].x, b, acc[4 * q + 0], 0, 0, 0);
                    acc[4 * q + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(m[q].y, b, acc[4 * q + 1], 0, 0, 0);
                    acc[4 * q + 2] = __builtin_amdgcn_mfma_f32_16x16x4f32(m[q].z, b, acc[4 * q + 2], 0, 0, 0);
                    acc[4 * q + 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(m[q].w, b, acc[4 * q + 3], 0, 0, 0);
                }
            };
            // TWO blocks in flight ahead of the one being multiplied: with four waves per CU each pulling 6 KB per block
            // through the CU's vector-memory port a request comes back after well over the 24 x 32 = 768 cycles a
            // block's MFMAs take -- one block ahead left part of every round trip exposed (1.97 ms per launch, this:
            // 1.67).  Three register sets, the loop unrolled by three and branch-free (KB is a multiple of 3: wide_kb
            // pads the model with zero blocks, which add exact zeros); the accumulators stay in AGPRs throughout.
            request(mA, bA, 0);
            request(mB, bB, 1);
#pragma unroll 1
            for (int kb = 0; kb < KB; kb += 3) {
                request(mC, bC, kb + 2);
                block(mA, bA);
                request(mA, bA, kb + 3);
                block(mB, bB);
                request(mB, bB, kb + 4);
                block(mC, bC);
            }
            // new observation: lane (j, g) holds columns 16 ct + 4 g .. + 3 of trajectory j (columns >= o: the model's
            // zero padding, they stay 0 for the linear model and tanh(0) = 0)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int ct = 0; ct < NT; ++ct) {
                f32x4 v = acc[ct];
                if (KIND == 1) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] = fast_tanh(v[k]);
                }
                const int col = 16 * ct + 4 * g;
                if (col < o) *reinterpret_cast<f32x4*>(X + j * XS + col) = v;
            }
            // (a last column group that straddles o also zeroes the first action slots: they are reloaded next step)
            if (diff) {   // the term that reads the observation just written
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                float c_step = 0.f;
                if (lane < 16) c_step = park[wave][lane] + wide_diff_cost(cs_s, X[lane * XS + cs_s.diff_idx], park[wave][16 + lane]);
                acc_c = wide_accumulate(acc_c, c_step, t, a.cost_mode);
            }
        }
        const float cost = acc_c;
        const int row = row0 + (lane & 15);
        const bool live = row < a.n_rows;
        if (live && lane < 16) a.costs[row] = cost;
        if (a.K > 0) {
            const unsigned long long key = (lane < 16 && live && row < a.n_cand) ? make_key(cost, row) : KEY_SENTINEL;
            run_key = topk_push16(run_key, key, first, a.K, lane);
            first = false;
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (a.K > 0) {
        FastRolloutArgs fr{};  // wg_merge_emit only looks at the candidate outputs
        fr.part_k = a.part_k;
        fr.part_c = a.part_c;
        fr.part_i = a.part_i;
        wg_merge_emit<WAVES>(wg_keys, run_key, a.K, lane, wave, fr);
    }
