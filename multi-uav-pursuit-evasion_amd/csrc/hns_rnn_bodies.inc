// hns_rnn_bodies.inc — the body of hns_rnn_actor_rows_kernel, which exists twice in hns_rnn_train.hip: for the shared head and for one head per
// agent (the stacked actor of share_actor: false; DESIGN.md §7.18).  Included as text, as hns_policy_train_bodies.inc is, so that each kernel is
// compiled from its own statements: the shared kernel's code is what it was before the second existed.  `a` holds the head the workgroup runs
// (the agents kernel: the agent's slices).  The including kernel defines
//   RT_TRIP_ROWS                : the rows its trips cover (shared: all B L A; agents: the B L positions of the workgroup's agent)
//   RT_TRIP_FIRST, RT_TRIP_STEP : the workgroup's trips
//   RT_ROW(p)                   : the row index (b L + t) A + a at place p of that numbering (>= a.G.rows: past the end)
    __shared__ __align__(16) float red[kRtRows][kRtE];
    __shared__ double reds[kRtRows][9];
    const int tid = threadIdx.x, r = tid >> 3, g = tid & 7;
    float w[kRtAct][16], hb[kRtAct], ls[kRtAct];
    double iv[kRtAct];
#pragma unroll
    for (int i = 0; i < kRtAct; ++i) {
        rt_load(a.head_w + i * kRtE, g, w[i]);
        hb[i] = a.head_b[i];
        ls[i] = a.log_std[i];
        iv[i] = exp(-2.0 * (double)ls[i]);                      // 1 / sigma^2
    }
    float aw[kRtAct][16], ab[kRtAct], al[kRtAct];
    double aq = 0.0;
#pragma unroll
    for (int i = 0; i < kRtAct; ++i) {
        ab[i] = 0.0f;
        al[i] = 0.0f;
#pragma unroll
        for (int q = 0; q < 16; ++q) aw[i][q] = 0.0f;
    }
    const long long trips = (RT_TRIP_ROWS + kRtRows - 1) / kRtRows;
    for (long long trip = RT_TRIP_FIRST; trip < trips; trip += RT_TRIP_STEP) {
        const long long row = RT_ROW(trip * kRtRows + r);
        const RtRow R = rt_row(a.G, row);
        float y[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) y[q] = 0.0f;
        if (R.live) rt_load(a.G.y + R.yoff, g, y);
        // logp sums four terms of order 1; its rounding is the ratio's relative error, so the terms and their sum are fp64 from the fp32 mean
        float am[kRtAct], dl[kRtAct];
        double lp = 0.0;
#pragma unroll
        for (int i = 0; i < kRtAct; ++i) {
            const float mu = rt_dot(w[i], y) + hb[i];
            const float act = R.live ? a.action[R.idx * kRtAct + i] : mu;
            const double dm = (double)act - (double)mu, z2 = dm * dm * iv[i];
            am[i] = (float)(dm * iv[i]);                        // (a - mu) / sigma^2
            dl[i] = (float)z2;                                  // (a - mu)^2 / sigma^2
            lp += (-0.5 * z2 - (double)ls[i]) - 0.9189385332046727;   // log sqrt(2 pi)
        }
        float ratio = -1.0f, dlogp = 0.0f;                      // -1: the row is not part of the minibatch
        double q0 = 0.0;
        if (R.live) {
            const float adv = a.adv[R.idx];
            ratio = expf((float)(lp - (double)a.logp_old[R.idx]));
            const float rc = fminf(fmaxf(ratio, a.clip_lo), a.clip_hi);
            const float s1 = ratio * adv, s2 = rc * adv;
            const bool inside = ratio >= a.clip_lo && ratio <= a.clip_hi;
            const float wgt = (inside || s1 < s2) ? 1.0f : 0.0f;
            const double d1 = (double)ratio * (double)adv, d2 = (double)rc * (double)adv;
            q0 = d1 < d2 ? d1 : d2;
            dlogp = -(float)kRtAct * adv * ratio * wgt * a.inv_n;
        }
        float dy[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) dy[q] = 0.0f;
#pragma unroll
        for (int i = 0; i < kRtAct; ++i) {
            const float dmu = dlogp * am[i];
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                dy[q] = __builtin_fmaf(dmu, w[i][q], dy[q]);
                aw[i][q] += dmu * y[q];                         // d fc_mean.weight[i]
            }
            ab[i] += dmu;
            al[i] += dlogp * (dl[i] - 1.0f);
        }
        aq += q0;
        if (R.in) {
            rt_store(a.G.dy + R.yoff, g, dy);                   // a dead row's dy: zeros
            if (g == 0) {
                a.ratio[(row % a.G.LA) * a.B + row / a.G.LA] = ratio;        // [column (t, a)][segment b]: the ESS kernel reads a column contiguously
                if (R.live && a.logp_new) a.logp_new[row] = (float)lp;
            }
        }
    }
    double *part = a.part + (long long)blockIdx.x * kRtActorSlots;
#pragma unroll
    for (int i = 0; i < kRtAct; ++i) rt_flush(red, aw[i], part + i * kRtE, tid, r, g);
    if (g == 0) {
#pragma unroll
        for (int i = 0; i < kRtAct; ++i) {
            reds[r][i] = (double)ab[i];
            reds[r][kRtAct + i] = (double)al[i];
        }
        reds[r][8] = aq;
    }
    __syncthreads();
    if (tid < 9) {
        double s = 0.0;
        for (int rr = 0; rr < kRtRows; ++rr) s += reds[rr][tid];
        part[kRtAct * kRtE + tid] = s;
    }
