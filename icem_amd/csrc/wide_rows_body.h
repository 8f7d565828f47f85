// wide_rows_body.h -- the BODY of rollout_rows_wide_kernel (k_rollout_wide.hip), included textually into the by-value kernel and
// into rollout_rows_wide_batch_kernel (k_rollout_wide_batch.hip; see wide_rollout_body.h).  Expects: template parameter KIND and
// `a` (WideRowsArgs) in scope.  No include guard.
    __shared__ float x[2][448];  // [obs | action], double buffered over the steps
    const int c = threadIdx.x, o = a.o, d = a.d, H = a.h;
    const int row = a.row0 + blockIdx.x;
    x[0][c] = c < o ? a.obs0[c] : 0.f;
    __shared__ CostArgs<float> cs_s;
    const bool ext = a.cs != nullptr;
    wide_stage_terms(cs_s, a.cs, threadIdx.x, 384);
    const bool sweep = ext && cs_s.health_idx >= 0, diff = ext && cs_s.diff_idx >= 0;
    float acc_c = 0.f, c_step = 0.f, dold = 0.f;
    for (int t = 0; t < H; ++t) {
        float* xc = x[t & 1];
        if (c < d) xc[o + c] = a.actions[((size_t)row * H + t) * d + c];
        __syncthreads();
        if (c == 0 && t > 0) {   // the previous step's cost is complete now that its next observation is visible
            if (diff) c_step += wide_diff_cost(cs_s, xc[cs_s.diff_idx], dold);
            acc_c = wide_accumulate(acc_c, c_step, t - 1, a.cost_mode);
        }
        bool bad = false;
        if (sweep) bad = __syncthreads_or(c < o && wide_bad_entry(cs_s, xc[c], c)) != 0;
        if (c == 0) c_step = wide_step_cost(a.wc, ext, cs_s, xc, o, d, bad, dold);   // rollout_wide_kernel's expression
        if (c < o) {
            float acc = 0.f;
            const float* Ac = a.A + c;
#pragma unroll 8
            for (int k = 0; k < o; ++k) acc = __builtin_fmaf(Ac[(size_t)k * o], xc[k], acc);
            const float* Bc = a.B + c;
#pragma unroll 4
            for (int k = 0; k < d; ++k) acc = __builtin_fmaf(Bc[(size_t)k * o], xc[o + k], acc);
            x[(t & 1) ^ 1][c] = KIND == 1 ? fast_tanh(acc) : acc;
        }
    }
    __syncthreads();
    if (c == 0) {
        if (diff) c_step += wide_diff_cost(cs_s, x[H & 1][cs_s.diff_idx], dold);
        a.costs[row] = wide_accumulate(acc_c, c_step, H - 1, a.cost_mode);
    }
