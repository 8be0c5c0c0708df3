// hns_gru_bodies.inc — the bodies of three kernels of hns_gru.hip that exist twice: for one GRU and for one GRU per agent (the stacked actor of
// share_actor: false; DESIGN.md §7.18).  Included as text, as hns_policy_train_bodies.inc is, so that each kernel is compiled from its own
// statements: the shared kernels' code is what it was before the second set existed.  The including kernel defines the macros that say where
// the two differ; `a` is the GruArgs of the network the workgroup runs (the agents kernels: the agent's slices, gru_agent_args).
//   GRU_TILE_FIRST, GRU_TILE_STEP : the workgroup's tiles
//   GRU_SEQ(p)                    : the sequence at position p of the tile numbering (shared: p itself; agents: b = p of the agent, p inner + agent)
//   GRU_LIVE(p, q)                : whether position p, sequence q, exists
//   GRU_GATE_SEQ                  : the column's sequence in the numbering of the gate gradients `a.dgate` points at
//   GRU_WG_RANGE, GRU_WG_HROW     : the weight-gradient workgroup's row range; a row's index into h_hist and is_init (from q and st)
#if defined(GRU_BODY_FWD)
    __shared__ __align__(16) GruLds L;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, col = lane & 15, kq = lane >> 4;
    const int u0 = 16 * w + 4 * kq;                             // the lane's four units
    GruWeights W;
    gru_load_weights(a, w, col, kq, W);
    const int Ls = a.L;
    for (int tile = GRU_TILE_FIRST; tile < a.tiles; tile += GRU_TILE_STEP) {
        const long long q0 = (long long)tile * kGruTile, qc = GRU_SEQ(q0 + col), qs = GRU_SEQ(q0 + (tid & 15));
        const bool valid = GRU_LIVE(q0 + col, qc);
        const long long xoff = valid ? gru_seq_off(a, qc) : 0;
        const float *xrow = GRU_LIVE(q0 + (tid & 15), qs) ? a.x + gru_seq_off(a, qs) : nullptr;
        f32x4 h = (valid && a.h0) ? *reinterpret_cast<const f32x4 *>(a.h0 + qc * kGruH + u0) : f32x4{0.f, 0.f, 0.f, 0.f};
        for (int t = 0; t < Ls; ++t) {
            const float m = (valid && a.is_init && a.is_init[qc * Ls + t]) ? 0.0f : 1.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r) h[r] = h[r] * m;
            gru_stage(L, a, xrow, t, tid, u0, col, h);
            __syncthreads();
            f32x4 acc[4];
            gru_gates(L, W, a, w, u0, col, kq, acc);
            f32x4 y;
            float s1 = 0.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float rg = gru_sigm(acc[0][r]), zg = gru_sigm(acc[1][r]), ng = tanhf(acc[2][r] + rg * acc[3][r]);
                h[r] = (1.0f - zg) * ng + zg * h[r];
                y[r] = h[r] + L.xs[gru_xslot(u0 + r) * kGruTile + col];
                s1 += y[r];
            }
            const float mean = gru_unit_sum(L, 0, s1, w, col, kq) * (1.0f / kGruH);
            float s2 = 0.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                y[r] = y[r] - mean;
                s2 += y[r] * y[r];
            }
            const float rstd = 1.0f / sqrtf(gru_unit_sum(L, 1, s2, w, col, kq) * (1.0f / kGruH) + kGruEps);
            if (valid) {
                const f32x4 lw = *reinterpret_cast<const f32x4 *>(a.ln_w + u0), lb = *reinterpret_cast<const f32x4 *>(a.ln_b + u0);
                f32x4 o;
#pragma unroll
                for (int r = 0; r < 4; ++r) o[r] = (y[r] * rstd) * lw[r] + lb[r];
                *reinterpret_cast<f32x4 *>(a.out + xoff + (long long)t * a.s2 + u0) = o;
                if (a.h_hist) *reinterpret_cast<f32x4 *>(a.h_hist + (qc * Ls + t) * kGruH + u0) = h;
            }
        }
        if (valid) *reinterpret_cast<f32x4 *>(a.h_last + qc * kGruH + u0) = h;
        __syncthreads();                                        // (the next tile's staging rewrites the LDS)
    }
#elif defined(GRU_BODY_BWD)
    __shared__ __align__(16) GruBwdLds B;
    GruLds &L = B.f;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, col = lane & 15, kq = lane >> 4;
    const int u0 = 16 * w + 4 * kq;
    GruWeights W;
    gru_load_weights(a, w, col, kq, W);
    const int Ls = a.L;
    f32x4 dlnw = f32x4{0.f, 0.f, 0.f, 0.f}, dlnb = f32x4{0.f, 0.f, 0.f, 0.f};      // the lane's sequence only; summed over the lanes at the end
    for (int tile = GRU_TILE_FIRST; tile < a.tiles; tile += GRU_TILE_STEP) {
        const long long q0 = (long long)tile * kGruTile, qc = GRU_SEQ(q0 + col), qs = GRU_SEQ(q0 + (tid & 15));
        const bool valid = GRU_LIVE(q0 + col, qc);
        const long long xoff = valid ? gru_seq_off(a, qc) : 0;
        const float *xrow = GRU_LIVE(q0 + (tid & 15), qs) ? a.x + gru_seq_off(a, qs) : nullptr;
        f32x4 dh = (valid && a.dh_last) ? *reinterpret_cast<const f32x4 *>(a.dh_last + qc * kGruH + u0) : f32x4{0.f, 0.f, 0.f, 0.f};
        for (int t = Ls - 1; t >= 0; --t) {
            f32x4 hp = f32x4{0.f, 0.f, 0.f, 0.f};
            if (valid) {
                if (t > 0) hp = *reinterpret_cast<const f32x4 *>(a.hist + (qc * Ls + t - 1) * kGruH + u0);
                else if (a.h0) hp = *reinterpret_cast<const f32x4 *>(a.h0 + qc * kGruH + u0);
            }
            const float m = (valid && a.is_init && a.is_init[qc * Ls + t]) ? 0.0f : 1.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r) hp[r] = hp[r] * m;
            gru_stage(L, a, xrow, t, tid, u0, col, hp);
            __syncthreads();
            f32x4 acc[4];
            gru_gates(L, W, a, w, u0, col, kq, acc);
            f32x4 rg, zg, ng, xh;
            float s1 = 0.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                rg[r] = gru_sigm(acc[0][r]);
                zg[r] = gru_sigm(acc[1][r]);
                ng[r] = tanhf(acc[2][r] + rg[r] * acc[3][r]);
                const float hn = (1.0f - zg[r]) * ng[r] + zg[r] * hp[r];
                xh[r] = hn + L.xs[gru_xslot(u0 + r) * kGruTile + col];
                s1 += xh[r];
            }
            const float mean = gru_unit_sum(L, 0, s1, w, col, kq) * (1.0f / kGruH);
            float s2 = 0.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                xh[r] = xh[r] - mean;
                s2 += xh[r] * xh[r];
            }
            const float rstd = 1.0f / sqrtf(gru_unit_sum(L, 1, s2, w, col, kq) * (1.0f / kGruH) + kGruEps);
            // LayerNorm backward: dy = rstd (g - mean(g) - xhat mean(g xhat)), g = dout ln_w
            const f32x4 dout = valid ? *reinterpret_cast<const f32x4 *>(a.dout + xoff + (long long)t * a.s2 + u0) : f32x4{0.f, 0.f, 0.f, 0.f};
            const f32x4 lw = *reinterpret_cast<const f32x4 *>(a.ln_w + u0);
            f32x4 g;
            float sg = 0.0f, sgx = 0.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                xh[r] = xh[r] * rstd;
                g[r] = dout[r] * lw[r];
                sg += g[r];
                sgx += g[r] * xh[r];
                dlnw[r] += dout[r] * xh[r];
                dlnb[r] += dout[r];
            }
            // (two sums behind one barrier: the slots differ)
            sg += __shfl_xor(sg, 16, 64);
            sg += __shfl_xor(sg, 32, 64);
            sgx += __shfl_xor(sgx, 16, 64);
            sgx += __shfl_xor(sgx, 32, 64);
            if (kq == 0) {
                L.red[2][w][col] = sg;
                L.red[3][w][col] = sgx;
            }
            __syncthreads();
            float mg = L.red[2][0][col], mgx = L.red[3][0][col];
#pragma unroll
            for (int k = 1; k < kGruWaves; ++k) {
                mg += L.red[2][k][col];
                mgx += L.red[3][k][col];
            }
            mg *= 1.0f / kGruH;
            mgx *= 1.0f / kGruH;
            f32x4 dy, dhz, dar, daz, dan, dahn;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                dy[r] = rstd * ((g[r] - mg) - xh[r] * mgx);
                const float dht = dh[r] + dy[r];                // d h_t: from the steps after t, and from out_t
                const float dn = dht * (1.0f - zg[r]), dz = dht * (hp[r] - ng[r]);
                dan[r] = dn * (1.0f - ng[r] * ng[r]);
                daz[r] = dz * (zg[r] * (1.0f - zg[r]));
                dar[r] = (dan[r] * acc[3][r]) * (rg[r] * (1.0f - rg[r]));
                dahn[r] = dan[r] * rg[r];
                dhz[r] = dht * zg[r];
                const int e = (u0 + r) * kGruTile + col;
                B.da[0][e] = dar[r];
                B.da[1][e] = daz[r];
                B.da[2][e] = dan[r];
                B.da[3][e] = dahn[r];
            }
            if (valid) {
                float *dg = a.dgate + (GRU_GATE_SEQ * Ls + t) * kGruGate + u0;
                *reinterpret_cast<f32x4 *>(dg) = dar;
                *reinterpret_cast<f32x4 *>(dg + kGruH) = daz;
                *reinterpret_cast<f32x4 *>(dg + 2 * kGruH) = dan;
                *reinterpret_cast<f32x4 *>(dg + 3 * kGruH) = dahn;
            }
            __syncthreads();
            // dx_t = W_ih^T dA_i, dh_{t-1} = W_hh^T dA_h for the wave's 16 units: k = gate row j = 4 s + kq over all 384 rows
            f32x4 dxa = f32x4{0.f, 0.f, 0.f, 0.f}, dha = f32x4{0.f, 0.f, 0.f, 0.f};
            const float *wi = a.w_ih + 16 * w + col, *wh = a.w_hh + 16 * w + col;
#pragma unroll 8
            for (int s = 0; s < 96; ++s) {
                const int j = 4 * s + kq, gt = s >> 5, e = (j & (kGruH - 1)) * kGruTile + col;
                const float bi = B.da[gt][e], bh = gt == 2 ? B.da[3][e] : bi;
                dxa = gru_mfma(wi[(long long)j * kGruH], bi, dxa);
                dha = gru_mfma(wh[(long long)j * kGruH], bh, dha);
            }
            if (valid) {
                f32x4 dxv;
#pragma unroll
                for (int r = 0; r < 4; ++r) dxv[r] = dxa[r] + dy[r];
                *reinterpret_cast<f32x4 *>(a.dx + xoff + (long long)t * a.s2 + u0) = dxv;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) dh[r] = (dha[r] + dhz[r]) * m;
        }
        if (valid && a.dh0) *reinterpret_cast<f32x4 *>(a.dh0 + qc * kGruH + u0) = dh;
        __syncthreads();
    }
    // this workgroup's LayerNorm partials: over the 16 sequences (lanes col = 0 .. 15 of this kq), fixed butterfly
    float *lp = a.lnpart + (long long)blockIdx.x * (2 * kGruH);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float sw = dlnw[r], sb = dlnb[r];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
            sw += __shfl_xor(sw, o, 64);
            sb += __shfl_xor(sb, o, 64);
        }
        if (col == 0) {
            lp[u0 + r] = sw;
            lp[kGruH + u0 + r] = sb;
        }
    }
#elif defined(GRU_BODY_WGRAD)
    __shared__ __align__(16) float sdy[kGruWgRows * kGruWgLd];
    __shared__ __align__(16) float sxx[kGruWgRows * kGruWgLd];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, col = lane & 15, kq = lane >> 4;
    const int m = blockIdx.y, split = blockIdx.x;
    const int blk = m < 3 ? m : (m == 5 ? 3 : m - 3);
    const int t0 = GRU_WG_RANGE * tps, t1 = t0 + tps < tiles ? t0 + tps : tiles;
    f32x4 acc[2][8];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[i][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bs0 = 0.0f, bs1 = 0.0f;
    for (int t = t0; t < t1; ++t) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + 256 * i, rr = idx >> 5, c4 = idx & 31;
            const long long row = (long long)t * kGruWgRows + rr;
            f32x4 dv = f32x4{0.f, 0.f, 0.f, 0.f}, ov = f32x4{0.f, 0.f, 0.f, 0.f};
            if (row < rows) {
                dv = *reinterpret_cast<const f32x4 *>(a.dgate + row * kGruGate + blk * kGruH + 4 * c4);
                const long long p = row / a.L;
                const int st = (int)(row - p * a.L);
                const long long q = GRU_SEQ(p);
                if (m < 3) {
                    ov = *reinterpret_cast<const f32x4 *>(a.x + gru_seq_off(a, q) + (long long)st * a.s2 + 4 * c4);
                } else {
                    if (st > 0) ov = *reinterpret_cast<const f32x4 *>(a.hist + (GRU_WG_HROW - 1) * kGruH + 4 * c4);
                    else if (a.h0) ov = *reinterpret_cast<const f32x4 *>(a.h0 + q * kGruH + 4 * c4);
                    const float mk = (a.is_init && a.is_init[GRU_WG_HROW]) ? 0.0f : 1.0f;
#pragma unroll
                    for (int j = 0; j < 4; ++j) ov[j] = ov[j] * mk;
                }
            }
            *reinterpret_cast<f32x4 *>(&sdy[rr * kGruWgLd + 4 * c4]) = dv;
            *reinterpret_cast<f32x4 *>(&sxx[rr * kGruWgLd + 4 * c4]) = ov;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const int k = 4 * s + kq;
            const float a0 = sdy[k * kGruWgLd + (2 * w) * 16 + col], a1 = sdy[k * kGruWgLd + (2 * w + 1) * 16 + col];
            bs0 += a0;
            bs1 += a1;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const float b = sxx[k * kGruWgLd + c * 16 + col];
                acc[0][c] = gru_mfma(a0, b, acc[0][c]);
                acc[1][c] = gru_mfma(a1, b, acc[1][c]);
            }
        }
        __syncthreads();
    }
    float *out = part + ((long long)split * 6 + m) * kGruWgOut;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int c = 0; c < 8; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) out[((2 * w + i) * 16 + 4 * kq + r) * kGruH + c * 16 + col] = acc[i][c][r];
    bs0 += __shfl_xor(bs0, 16, 64);
    bs0 += __shfl_xor(bs0, 32, 64);
    bs1 += __shfl_xor(bs1, 16, 64);
    bs1 += __shfl_xor(bs1, 32, 64);
    if (kq == 0) {
        out[kGruMat + (2 * w) * 16 + col] = bs0;
        out[kGruMat + (2 * w + 1) * 16 + col] = bs1;
    }
#endif
