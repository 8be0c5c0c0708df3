// hns_policy_train_bodies.inc — the bodies of two kernels of hns_policy_train.hip that exist twice: for the shared networks and for one actor per
// agent (share_actor: false; DESIGN.md §7.16).  Included as text, so that each kernel is compiled from its own statements: the shared kernels'
// code is what it was before the second pair existed.  The including kernel defines the macros that say where the two differ.
#if defined(CT_BODY_TILE)
// A tile kernel's body.  CT_TILE_BLOCK: the tile's number (its staging block, partial rows, loss partials); CT_TILE_ROW: the thread's row of the
// minibatch, position x A + agent (from `tile` and `r`; >= a.rows: not live); CT_TILE_FIRST, CT_TILE_STEP: the tile's rows of agent `ag` for the
// ratios' partials.  `a.img` and `a.net` are the network the tile runs.  The per-row arithmetic knows none of this.
// CT_CENTRAL (the centralised critic, HEAD = 1; DESIGN.md §7.20) switches, by the preprocessor, so that every other kernel keeps its statements:
// a row is an env-step (ct_row_central), tokens 1 .. A - 1 are state_drones rows through token 0's embedding (ct_token_j_central), the head has
// A rows (the row's A values, A loss terms and A value gradients), and d embed_self is summed over all A drone tokens (ct_embed_self_sums).
    static_assert(HEAD == 0 || HEAD == 1 || (HEAD == kActDim && BWD), "the actor's head runs in the one-pass kernel");
    extern __shared__ __align__(16) unsigned char lds_raw[];
    CtLds &L = *reinterpret_cast<CtLds *>(lds_raw);
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r = tid >> 3, g = tid & 7;
    const float *img = a.img;
    const EncNet &N = a.net;
    const int ntok = a.A + a.K;
    float *part = BWD ? a.tilepart + (long long)CT_TILE_BLOCK * 2 * a.P : nullptr;

    {   // one tile per workgroup: its two partial rows are written, never accumulated
        const int tile = CT_TILE_BLOCK;
        const long long row = CT_TILE_ROW;
#if defined(CT_CENTRAL)
        const CtRow R = ct_row_central(a, row);
#define CT_TOKEN_J ct_token_j_central
#else
        const CtRow R = ct_row(a, row);
#define CT_TOKEN_J ct_token_j
#endif
        float *stg = BWD ? a.stage + (long long)tile * kCtRows * kCtE : nullptr;
        const long long SA = a.stage_rows * kCtE;               // floats per staging array

        // ---- forward
        float t[16], xh[16];
        ct_token(img + I_EW, N.eb[0], R.xs, a.D, N, g, xh, t);                 // token 0
        enc_lds_store(L.a, r, g, t);
        if (BWD) crow_store(stg + 1 * SA, kCtE, r, g, t);
        __syncthreads();
        enc_matvec<0>(img + 0 * kCtMat, N.in_b, L.a, L.b, nullptr, BWD ? stg + 2 * SA : nullptr, w, lane);          // q
        __syncthreads();
        enc_matvec<2>(img + 1 * kCtMat, nullptr, L.b, L.c, nullptr, nullptr, w, lane);       // W_k^T q / sqrt(128)
        __syncthreads();
        float kq[16], z[16];
        enc_lds_load(L.c, r, g, kq);
        float s, m = enc_score(kq, t), l = 1.0f;
        const float s0 = m;
#pragma unroll
        for (int i = 0; i < 16; ++i) z[i] = t[i];
        for (int j = 1; j < ntok; ++j) {
            const float *x;
            int n;
            CT_TOKEN_J(a, R, j, g, xh, t, x, n);
            enc_softmax_step(kq, t, m, l, z);
        }
        const float il = 1.0f / l;
#pragma unroll
        for (int i = 0; i < 16; ++i) z[i] *= il;
        enc_lds_store(L.b, r, g, z);
        if (BWD) crow_store(stg + 5 * SA, kCtE, r, g, z);
        __syncthreads();
        enc_matvec<0>(img + 2 * kCtMat, N.in_b + 2 * kCtE, L.b, L.c, nullptr, BWD ? stg + 7 * SA : nullptr, w, lane);   // v = W_v z + b_v
        __syncthreads();
        enc_matvec<0>(img + 3 * kCtMat, N.out_b, L.c, L.b, nullptr, nullptr, w, lane);       // attn
        __syncthreads();
        float x1[16], xh1[16], u[16];
        enc_lds_load(L.a, r, g, u);
        enc_lds_load(L.b, r, g, t);
#pragma unroll
        for (int i = 0; i < 16; ++i) u[i] += t[i];
        const float rstd1 = enc_layernorm(u, N.n1_w, N.n1_b, g, xh1, x1);                           // x0' = LN1(x0 + attn)
        enc_lds_store(L.a, r, g, x1);
        if (BWD) crow_store(stg + 9 * SA, kCtE, r, g, x1);
        __syncthreads();
        if (BWD) enc_matvec<4>(img + 4 * kCtMat, N.l1_b, L.a, L.b, L.p, stg + 11 * SA, w, lane);   // h = gelu(W_1 x0' + b_1), the pre-activation to p
        else enc_matvec<1>(img + 4 * kCtMat, N.l1_b, L.a, L.b, nullptr, nullptr, w, lane);
        __syncthreads();
        enc_matvec<0>(img + 5 * kCtMat, N.l2_b, L.b, L.c, nullptr, nullptr, w, lane);        // W_2 h + b_2
        __syncthreads();
        float y[16], xh2[16];
        enc_lds_load(L.c, r, g, t);
#pragma unroll
        for (int i = 0; i < 16; ++i) u[i] = x1[i] + t[i];
        const float rstd2 = enc_layernorm(u, N.n2_w, N.n2_b, g, xh2, y);                            // y = LN2(x0' + ff)
        float dv = 0.0f, dmu[HEAD ? HEAD : 1];
        float dy[16], dw[16], db[16], dx[16];
#if defined(CT_CENTRAL)
        // ---- v_out = Linear(128, A) on the row's ONE feature vector: A values against the env-step's A old values and returns.  Value o is
        // the shared critic's statements on row o of the head; the first joins by assignment and the others by addition, so one agent
        // leaves the shared critic's bits.
        float dva[HNS_MAX_AGENTS];
        {
            float hw[16];
            double q0 = 0.0, q1 = 0.0, q2 = 0.0, q3 = 0.0, q4 = 0.0;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                dy[i] = 0.0f;
                dw[i] = 0.0f;
                db[i] = 0.0f;
            }
#pragma unroll
            for (int o = 0; o < HNS_MAX_AGENTS; ++o) {
                dva[o] = 0.0f;
                if (o >= a.A) continue;
                enc_vec_load(N.head_w + o * kCtE, g, hw);
                s = 0.0f;
#pragma unroll
                for (int i = 0; i < 16; ++i) s = __builtin_fmaf(hw[i], y[i], s);
                const float v = row_sum8(s) + N.head_b[o];
                float ret = 0.0f, bv = 0.0f;
                if (R.live) {
                    ret = a.bret[R.e * a.A + o];
                    bv = a.bval[R.e * a.A + o];
                }
                const float d = v - bv;
                const float dcl = fminf(fmaxf(d, -a.clip), a.clip);
                const float clipped = bv + dcl;
                if (!BWD) {
                    if (g == 0 && R.live) {
                        if (a.values) a.values[row * a.A + o] = v;
                        const double e0 = (double)v - (double)ret, e1 = (double)clipped - (double)ret;
                        const double l0 = ct_loss64(e0, (double)a.delta, a.mse), l1 = ct_loss64(e1, (double)a.delta, a.mse);
                        q0 = o == 0 ? l0 : q0 + l0;
                        q1 = o == 0 ? l1 : q1 + l1;
                        q2 = o == 0 ? e0 * e0 : q2 + e0 * e0;
                        q3 = o == 0 ? (double)ret : q3 + (double)ret;
                        q4 = o == 0 ? (double)ret * (double)ret : q4 + (double)ret * (double)ret;
                    }
                } else {
                    if (R.live) {
                        const float g0 = ct_dloss(v - ret, a.delta, a.mse);
                        const float g1 = (d >= -a.clip && d <= a.clip) ? ct_dloss(clipped - ret, a.delta, a.mse) : 0.0f;
                        dva[o] = (a.ctl[0] * g0 + a.ctl[1] * g1) * a.inv_n;
                    }
#pragma unroll
                    for (int i = 0; i < 16; ++i) dy[i] = o == 0 ? dva[o] * hw[i] : __builtin_fmaf(dva[o], hw[i], dy[i]);
                }
            }
            if (!BWD) {
                if (g == 0) {
                    L.dred[0 * kCtRows + r] = q0; L.dred[1 * kCtRows + r] = q1; L.dred[2 * kCtRows + r] = q2;
                    L.dred[3 * kCtRows + r] = q3; L.dred[4 * kCtRows + r] = q4;
                }
                __syncthreads();
                if (tid < 5) {
                    double acc = 0.0;
                    for (int rr = 0; rr < kCtRows; ++rr) acc += L.dred[tid * kCtRows + rr];
                    a.losspart[(long long)tile * 5 + tid] = acc;
                }
                return;
            }
        }
#else
        if constexpr (HEAD == 0) {
            // ---- the encoder op: the features leave, or d features arrive, as [rows, 128]; a row that is not live is neither written nor read
            if (!BWD) {
                if (R.live) crow_store(a.feat + row * kCtE, kCtE, 0, g, y);
                return;
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                dy[i] = 0.0f;
                dw[i] = 0.0f;
                db[i] = 0.0f;
            }
            if (R.live) enc_vec_load(a.dfeat + row * kCtE, g, dy);
        } else if constexpr (HEAD == 1) {
            float hw[16];
            enc_vec_load(N.head_w, g, hw);
            s = 0.0f;
#pragma unroll
            for (int i = 0; i < 16; ++i) s = __builtin_fmaf(hw[i], y[i], s);
            const float v = row_sum8(s) + N.head_b[0];
            float ret = 0.0f, bv = 0.0f;
            if (R.live) {
                ret = a.bret[R.e * a.A + R.ag];
                bv = a.bval[R.e * a.A + R.ag];
            }
            const float d = v - bv;
            const float dcl = fminf(fmaxf(d, -a.clip), a.clip);
            const float clipped = bv + dcl;

            if (!BWD) {
                if (g == 0) {
                    double q0 = 0.0, q1 = 0.0, q2 = 0.0, q3 = 0.0, q4 = 0.0;
                    if (R.live) {
                        if (a.values) a.values[row] = v;
                        const double e0 = (double)v - (double)ret, e1 = (double)clipped - (double)ret;
                        q0 = ct_loss64(e0, (double)a.delta, a.mse);
                        q1 = ct_loss64(e1, (double)a.delta, a.mse);
                        q2 = e0 * e0;
                        q3 = (double)ret;
                        q4 = (double)ret * (double)ret;
                    }
                    L.dred[0 * kCtRows + r] = q0; L.dred[1 * kCtRows + r] = q1; L.dred[2 * kCtRows + r] = q2;
                    L.dred[3 * kCtRows + r] = q3; L.dred[4 * kCtRows + r] = q4;
                }
                __syncthreads();
                if (tid < 5) {
                    double acc = 0.0;
                    for (int rr = 0; rr < kCtRows; ++rr) acc += L.dred[tid * kCtRows + rr];
                    a.losspart[(long long)tile * 5 + tid] = acc;
                }
                return;
            }

            // ---- backward: dv from the branch weights of max(mean loss(v), mean loss(clipped))
            if (R.live) {
                const float g0 = ct_dloss(v - ret, a.delta, a.mse);
                const float g1 = (d >= -a.clip && d <= a.clip) ? ct_dloss(clipped - ret, a.delta, a.mse) : 0.0f;   // clamp's backward: inside, bounds included
                dv = (a.ctl[0] * g0 + a.ctl[1] * g1) * a.inv_n;
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                dy[i] = dv * hw[i];
                u[i] = dv * y[i];                                   // d head_w
                dw[i] = 0.0f;
                db[i] = 0.0f;
            }
        } else {
            // ---- the actor's head: mu = fc_mean(y), Normal(mu, exp(log_std)).log_prob(action) summed, the ratio and the clipped surrogate;
            // d logp = -k adv r w / n with w per row (1 inside the clip, bounds included; outside 1 where the unclipped surrogate is the smaller)
            // logp sums four terms of order 1 to a number of order 10 whose ROUNDING is the ratio's relative error (r = exp(logp - logp_old)): the terms
            // and their sum are formed in fp64 from the fp32 mean, so the ratio carries the mean's error only
            float am[HEAD], dls[HEAD], hr[16];
            double lp = 0.0;
#pragma unroll
            for (int i = 0; i < HEAD; ++i) {
                enc_vec_load(N.head_w + i * kCtE, g, hr);              // fc_mean.weight's row, read again in the backward pass (not kept)
                s = 0.0f;
#pragma unroll
                for (int q = 0; q < 16; ++q) s = __builtin_fmaf(hr[q], y[q], s);
                const float mu = row_sum8(s) + N.head_b[i];
                const float ls = N.log_std[i];
                const double iv = exp(-2.0 * (double)ls);                          // 1 / sigma^2
                const float act = R.live ? a.action[(R.e * a.A + R.ag) * HEAD + i] : mu;
                const double dm = (double)act - (double)mu, z2 = dm * dm * iv;
                am[i] = (float)(dm * iv);                                          // (a - mu) / sigma^2
                dls[i] = (float)z2;                                                // (a - mu)^2 / sigma^2
                lp += (-0.5 * z2 - (double)ls) - 0.9189385332046727;               // log sqrt(2 pi)
            }
            const float logp = (float)lp;
            float ratio = -1.0f, dlogp = 0.0f;
            double q0 = 0.0;
            if (R.live) {
                const float adv = a.adv[R.e * a.A + R.ag];
                ratio = expf((float)(lp - (double)a.logp_old[R.e * a.A + R.ag]));
                const float rc = fminf(fmaxf(ratio, a.clip_lo), a.clip_hi);
                const float s1 = ratio * adv, s2 = rc * adv;
                const bool inside = ratio >= a.clip_lo && ratio <= a.clip_hi;
                const float wgt = (inside || s1 < s2) ? 1.0f : 0.0f;
                const double d1 = (double)ratio * (double)adv, d2 = (double)rc * (double)adv;
                q0 = d1 < d2 ? d1 : d2;
                dlogp = -(float)HEAD * adv * ratio * wgt * a.inv_n;
            }
#pragma unroll
            for (int i = 0; i < HEAD; ++i) {
                dmu[i] = dlogp * am[i];
                dls[i] = dlogp * (dls[i] - 1.0f);
            }
            if (g == 0) {
                if (R.live && a.logp_new) a.logp_new[row] = logp;
                L.dred[0 * kCtRows + r] = q0;
                L.dred[1 * kCtRows + r] = (double)ratio;            // -1: the row is not part of the minibatch
#pragma unroll
                for (int i = 0; i < HEAD; ++i) {
                    L.sx[i * kCtRows + r] = dmu[i];
                    L.sx[(HEAD + i) * kCtRows + r] = dls[i];
                }
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                dy[i] = 0.0f;
                dw[i] = 0.0f;
                db[i] = 0.0f;
            }
#pragma unroll
            for (int i = 0; i < HEAD; ++i) {
                enc_vec_load(N.head_w + i * kCtE, g, hr);
#pragma unroll
                for (int q = 0; q < 16; ++q) dy[q] = __builtin_fmaf(dmu[i], hr[q], dy[q]);
            }
        }
#endif
        ct_ln_bwd(dy, xh2, rstd2, N.n2_w, g, dx, dw, db);       // dx = d(x0' + ff)
        enc_lds_store(L.b, r, g, dx);
        crow_store(stg + 10 * SA, kCtE, r, g, dx);
#if defined(CT_CENTRAL)
#pragma unroll
        for (int o = 0; o < HNS_MAX_AGENTS; ++o) {               // d v_out.weight[o] = sum_rows dv_o y; the rows' dv_o wait in sx for d v_out.bias
            if (o >= a.A) continue;
            if (g == 0) L.sx[o * kCtRows + r] = dva[o];
#pragma unroll
            for (int i = 0; i < 16; ++i) u[i] = dva[o] * y[i];
            ct_flush(L, u, part, a.P, o == 0 ? O_HW : O_EWS + a.D * kCtE + (o - 1) * kCtE, tid, r, g);
        }
        if (tid < 2 * a.A) {                                    // d v_out.bias: the two halves' sums of each dv_o
            const int half = tid & 1, o = tid >> 1;
            float sb = 0.0f;
            for (int rr = 0; rr < 16; ++rr) sb += L.sx[o * kCtRows + half * 16 + rr];
            float *dst = part + (long long)half * a.P + ct_central_hb(a.D) + o;
            *dst = sb;
        }
#else
        if constexpr (HEAD == 1) {
            if (g == 0) L.sc[r] = dv;
            ct_flush(L, u, part, a.P, O_HW, tid, r, g);
        } else if constexpr (HEAD == kActDim) {
#pragma unroll
            for (int i = 0; i < HEAD; ++i) {                        // d fc_mean.weight[i] = sum_rows d mu_i y
#pragma unroll
                for (int q = 0; q < 16; ++q) u[q] = dmu[i] * y[q];
                ct_flush(L, u, part, a.P, i == 0 ? O_HW : O_EWS + a.D * kCtE + (i - 1) * kCtE, tid, r, g);
            }
            if (tid < 4 * HEAD) {                                   // d fc_mean.bias and the rows' part of d log_std: the two halves' sums
                const int half = tid & 1, q = tid >> 1;
                float sb = 0.0f;
                for (int rr = 0; rr < 16; ++rr) sb += L.sx[q * kCtRows + half * 16 + rr];
                float *dst = part + (long long)half * a.P + (q < HEAD ? O_HB + q : O_EWS + a.D * kCtE + (HEAD - 1) * kCtE + (q - HEAD));
                *dst = sb;
            } else if (tid >= 32 && tid < 32 + a.A) {               // the ratios of agent tid - 32: max, sum exp(r - max), sum exp(2 (r - max))
                const int ag = tid - 32;
                const int first = CT_TILE_FIRST, step = CT_TILE_STEP;     // the tile's rows of agent `ag`
                double mx = -1.0, e1 = 0.0, e2 = 0.0;
                for (int rr = first; rr < kCtRows; rr += step) mx = L.dred[kCtRows + rr] > mx ? L.dred[kCtRows + rr] : mx;
                for (int rr = first; rr < kCtRows; rr += step) {
                    const double x = L.dred[kCtRows + rr];
                    if (x >= 0.0 || x != x) {
                        const double ex = exp(x - mx);
                        e1 += ex;
                        e2 += ex * ex;
                    }
                }
                double *dst = a.losspart + (long long)tile * kActLossSlots + 1 + 3 * ag;
                dst[0] = mx; dst[1] = e1; dst[2] = e2;
            } else if (tid == 64) {
                double acc = 0.0;
                for (int rr = 0; rr < kCtRows; ++rr) acc += L.dred[rr];
                a.losspart[(long long)tile * kActLossSlots] = acc;
            }
        }
#endif
        ct_flush(L, dw, part, a.P, O_N2W, tid, r, g);
        ct_flush(L, db, part, a.P, O_N2B, tid, r, g);
#if !defined(CT_CENTRAL)
        if constexpr (HEAD == 1) {
            if ((tid & 127) == 0) {                                 // d head_b: the two halves' sums of dv
                const int half = tid >> 7;
                float sb = 0.0f;
                for (int rr = 0; rr < 16; ++rr) sb += L.sc[half * 16 + rr];
                float *dst = part + (long long)half * a.P + O_HB;
                *dst = sb;
            }
        }
#endif
        enc_matvec<3>(img + 11 * kCtMat, nullptr, L.b, L.c, nullptr, nullptr, w, lane);      // dh = W_2^T dff
        __syncthreads();
        enc_lds_load(L.c, r, g, t);
        enc_lds_load(L.p, r, g, u);
#pragma unroll
        for (int i = 0; i < 16; ++i) {                          // gelu'(x) = Phi(x) + x phi(x)
            const float xx = u[i];
            const float dg = 0.5f * (1.0f + erff(xx * 0.7071067811865476f)) + xx * (0.3989422804014327f * expf(-0.5f * xx * xx));
            t[i] = t[i] * dg;
        }
        enc_lds_store(L.c, r, g, t);
        crow_store(stg + 8 * SA, kCtE, r, g, t);
        __syncthreads();
        enc_matvec<3>(img + 10 * kCtMat, nullptr, L.c, L.p, nullptr, nullptr, w, lane);      // W_1^T dh'
        __syncthreads();
        enc_lds_load(L.b, r, g, dy);
        enc_lds_load(L.p, r, g, t);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            dy[i] += t[i];                                      // d x0'
            dw[i] = 0.0f;
            db[i] = 0.0f;
        }
        ct_ln_bwd(dy, xh1, rstd1, N.n1_w, g, dx, dw, db);       // dx = d(x0 + attn)
        enc_lds_store(L.a, r, g, dx);
        crow_store(stg + 6 * SA, kCtE, r, g, dx);
        ct_flush(L, dw, part, a.P, O_N1W, tid, r, g);
        ct_flush(L, db, part, a.P, O_N1B, tid, r, g);
        enc_matvec<3>(img + 9 * kCtMat, nullptr, L.a, L.b, nullptr, stg + 4 * SA, w, lane);  // dv = W_o^T dattn
        __syncthreads();
        enc_matvec<3>(img + 8 * kCtMat, nullptr, L.b, L.c, nullptr, nullptr, w, lane);       // dz = W_v^T dv
        __syncthreads();

        // ---- token pass backward: alpha_j = exp(s_j - m) / l, ds_j = alpha_j (dz.t_j - dz.z), dt_j = alpha_j dz + ds_j kq
        float dz[16], dkq[16], dt0[16];
        enc_lds_load(L.c, r, g, dz);
        s = 0.0f;
#pragma unroll
        for (int i = 0; i < 16; ++i) s = __builtin_fmaf(dz[i], z[i], s);
        const float dzz = row_sum8(s);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            dw[i] = 0.0f;                                       // d ln_w, d ln_b over every token of the row
            db[i] = 0.0f;
        }
        {
            // token 0: its LayerNorm backward waits for W_q^T dq
            ct_token(img + I_EW, N.eb[0], R.xs, a.D, N, g, xh, t);
            s = 0.0f;
#pragma unroll
            for (int i = 0; i < 16; ++i) s = __builtin_fmaf(dz[i], t[i], s);
            const float al = expf(s0 - m) * il, ds = al * (row_sum8(s) - dzz);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                dt0[i] = __builtin_fmaf(ds, kq[i], al * dz[i]);
                dkq[i] = ds * t[i];
            }
        }
        float eo[4] = {0.f, 0.f, 0.f, 0.f}, ec[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // the thread's (feature, half) sums: bias, then the inputs
        const int ef = tid & 127, eh = tid >> 7;
        for (int j = 1; j < ntok; ++j) {
            const float *x;
            int n;
            const float rs = CT_TOKEN_J(a, R, j, g, xh, t, x, n);
            float sa = 0.0f, sd = 0.0f;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                sa = __builtin_fmaf(kq[i], t[i], sa);
                sd = __builtin_fmaf(dz[i], t[i], sd);
            }
            const float al = expf(row_sum8(sa) - m) * il, ds = al * (row_sum8(sd) - dzz);
            float dt[16], de[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                dt[i] = __builtin_fmaf(ds, kq[i], al * dz[i]);
                dkq[i] = __builtin_fmaf(ds, t[i], dkq[i]);
            }
            ct_ln_bwd(dt, xh, rs, N.ln_w, g, de, dw, db);
#if defined(CT_CENTRAL)
            if (j < a.A) {                                      // a drone token: the first of them writes the tile's d embed_self sums
                ct_embed_self_sums(L, de, x, a.D, part + (long long)eh * a.P, ef, eh, r, g, j > 1);
                continue;
            }
#endif
            crow_store(L.red, kCtRedLd, r, g, de);
            if (g < n) L.sx[g * kCtRows + r] = x ? x[g] : 0.0f;
            __syncthreads();
            if (j < a.A) {
#pragma unroll
                for (int rr = 0; rr < 16; ++rr) {
                    const int q = eh * 16 + rr;
                    const float dd = L.red[q * kCtRedLd + ef];
                    eo[0] += dd;
#pragma unroll
                    for (int k = 0; k < 3; ++k) eo[1 + k] = __builtin_fmaf(dd, L.sx[k * kCtRows + q], eo[1 + k]);
                }
            } else {
#pragma unroll
                for (int rr = 0; rr < 16; ++rr) {
                    const int q = eh * 16 + rr;
                    const float dd = L.red[q * kCtRedLd + ef];
                    ec[0] += dd;
#pragma unroll
                    for (int k = 0; k < 5; ++k) ec[1 + k] = __builtin_fmaf(dd, L.sx[k * kCtRows + q], ec[1 + k]);
                }
            }
            __syncthreads();
        }
        {
            float *ph = part + (long long)eh * a.P;
#if !defined(CT_CENTRAL)
            ph[O_EBO + ef] = eo[0];
#pragma unroll
            for (int k = 0; k < 3; ++k) ph[O_EWO + k * kCtE + ef] = eo[1 + k];
#endif
            ph[O_EBC + ef] = ec[0];
#pragma unroll
            for (int k = 0; k < 5; ++k) ph[O_EWC + k * kCtE + ef] = ec[1 + k];
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) dkq[i] *= 0.08838834764831845f;          // d(W_k^T q) = dkq / sqrt(128)
        enc_lds_store(L.b, r, g, dkq);
        crow_store(stg + 3 * SA, kCtE, r, g, dkq);
        __syncthreads();
        enc_matvec<3>(img + 7 * kCtMat, nullptr, L.b, L.c, nullptr, stg + 0 * SA, w, lane);  // dq = W_k d(W_k^T q)
        __syncthreads();
        enc_matvec<3>(img + 6 * kCtMat, nullptr, L.c, L.b, nullptr, nullptr, w, lane);       // W_q^T dq
        __syncthreads();
        {
            float de[16];
            enc_lds_load(L.a, r, g, u);
            enc_lds_load(L.b, r, g, y);
#pragma unroll
            for (int i = 0; i < 16; ++i) dt0[i] = (dt0[i] + u[i]) + y[i];
            const float rs = ct_token(img + I_EW, N.eb[0], R.xs, a.D, N, g, xh, t);
            ct_ln_bwd(dt0, xh, rs, N.ln_w, g, de, dw, db);
#if defined(CT_CENTRAL)
            ct_embed_self_sums(L, de, R.xs, a.D, part + (long long)eh * a.P, ef, eh, r, g, a.A > 1);     // the query drone joins the others'
#else
            crow_store(L.red, kCtRedLd, r, g, de);
            for (int k = g; k < a.D; k += 8) L.sx[k * kCtRows + r] = R.xs ? R.xs[k] : 0.0f;
            __syncthreads();
            float *ph = part + (long long)eh * a.P;
            float sb = 0.0f;
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) sb += L.red[(eh * 16 + rr) * kCtRedLd + ef];
            ph[O_EBS + ef] = sb;
            for (int k = 0; k < a.D; ++k) {
                float sw = 0.0f;
#pragma unroll
                for (int rr = 0; rr < 16; ++rr) sw = __builtin_fmaf(L.red[(eh * 16 + rr) * kCtRedLd + ef], L.sx[k * kCtRows + eh * 16 + rr], sw);
                ph[O_EWS + k * kCtE + ef] = sw;
            }
            __syncthreads();
#endif
        }
        ct_flush(L, dw, part, a.P, O_LNW, tid, r, g);
        ct_flush(L, db, part, a.P, O_LNB, tid, r, g);
    }
#undef CT_TOKEN_J
#elif defined(CT_BODY_LOSS)
// The actor's scalars.  CT_LOSS_NLS: the log_std vectors ([CT_LOSS_NLS][4]); CT_LOSS_ENTROPY: the rows' mean entropy from their sum `ent`.
    __shared__ double sm[kActLossSlots][64];
    const int tid = threadIdx.x;
    double acc = 0.0, mx[HNS_MAX_AGENTS], s1[HNS_MAX_AGENTS], s2[HNS_MAX_AGENTS];
#pragma unroll
    for (int q = 0; q < HNS_MAX_AGENTS; ++q) { mx[q] = -1.0; s1[q] = 0.0; s2[q] = 0.0; }
    for (int i = tid; i < tiles; i += 64) {
        const double *t = part + (long long)i * kActLossSlots;
        acc += t[0];
#pragma unroll
        for (int q = 0; q < HNS_MAX_AGENTS; ++q) {
            if (q >= A) continue;
            const double m = t[1 + 3 * q], e1 = t[2 + 3 * q], e2 = t[3 + 3 * q];
            if (e1 == 0.0) continue;                            // no row of this agent in the tile
            const double M = m > mx[q] ? m : mx[q];
            const double c0 = s1[q] == 0.0 ? 0.0 : exp(mx[q] - M), c1 = exp(m - M);
            s1[q] = s1[q] * c0 + e1 * c1;
            s2[q] = s2[q] * (c0 * c0) + e2 * (c1 * c1);
            mx[q] = M;
        }
    }
    sm[0][tid] = acc;
#pragma unroll
    for (int q = 0; q < HNS_MAX_AGENTS; ++q) { sm[1 + 3 * q][tid] = mx[q]; sm[2 + 3 * q][tid] = s1[q]; sm[3 + 3 * q][tid] = s2[q]; }
    __syncthreads();
    if (tid == 0) {
        double tot = 0.0;
        for (int i = 0; i < 64; ++i) tot += sm[0][i];
        policy_loss[0] = (float)(-(double)kActDim * tot / n);
        double ent = 0.0;
        for (int i = 0; i < CT_LOSS_NLS * kActDim; ++i) ent += 0.5 + 0.9189385332046727 + (double)log_std[i];
        entropy[0] = (float)CT_LOSS_ENTROPY;
        double es = 0.0;
        for (int q = 0; q < A; ++q) {
            double M = -1.0, a1 = 0.0, a2 = 0.0;
            for (int i = 0; i < 64; ++i) {
                const double m = sm[1 + 3 * q][i], e1 = sm[2 + 3 * q][i], e2 = sm[3 + 3 * q][i];
                if (e1 == 0.0) continue;
                const double Mn = m > M ? m : M;
                const double c0 = a1 == 0.0 ? 0.0 : exp(M - Mn), c1 = exp(m - Mn);
                a1 = a1 * c0 + e1 * c1;
                a2 = a2 * (c0 * c0) + e2 * (c1 * c1);
                M = Mn;
            }
            es += a1 * a1 / a2;                                 // exp(2 (M + log a1) - (2 M + log a2))
        }
        ess[0] = (float)(es / (double)A / batch);
    }
#endif
