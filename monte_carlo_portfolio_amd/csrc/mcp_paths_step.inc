// mcp_paths_step.inc -- one step t of the path kernels' walk (mcp_paths_body.inc, included in its step loops): the normals of
// step t, r = mu + L z (BOOT: r = row j_t of the observed returns), rho = w.r, the update of V (and, DD, of the running peak
// and drawdown state).  REB: no rho and no V; the returns since the last rebalance B_i = B_i + r_i + B_i r_i instead
// (SPEC.md 4.5), a = B + r then B = fma(B, r, a), one v_pk_add_f32 and one v_pk_fma_f32 per pair of assets.  STT: the step's
// chi blocks first (only s stays live while the asset normals are formed), then every asset normal scaled by s as it leaves
// block_normals (SPEC.md 2.2 / 4.6).  CF: the flow c_s after the update, ruin absorbing (SPEC.md 4.7).  OV: between the row pair's
// returns and the weight dot, the return of every asset that owns option rows is replaced by its rows' return at the asset's price
// level (SPEC.md 4.8); whether an asset owns rows is wave-uniform, a scalar branch.  GV: s is replaced by u = s sqrt(h) (nu = 0: u =
// sqrt(h), the chi blocks skipped by a scalar branch) and h is updated from the scaled normals (SPEC.md 4.9).  AT: between the row
// pair's returns and the weight dot, c = fl32(w r) and A = fma(V, c, A) for the pair, one v_pk_mul_f32 and one v_pk_fma_f32, V the
// value before this step's update (SPEC.md 4.10).  ANTI: the step's normals are formed once; the row pair's accumulator, rho and
// the update of V (DD: of the peak and drawdown) run for EM = 2 PPT members, member PPT + e on -z[e] (SPEC.md 2.3): a second fma
// chain from the same mu2 -- never a shared L z, mu + L z and mu - L z round differently.  FH: the gathered row is a residual, r_i = fma(sqrt(h),
// E_ji, mu_i) with mu from the packed block by scalar loads, and after the update of V h moves on the row's shock (SPEC.md 4.11).  In scope: everything mcp_paths_body.inc
// declares before its step loops, and t.  JP: one more Philox block on counter stream 3 before the asset normals gives
// the step's market jump J, and the row pair's accumulator starts at fma(b, J, mu) (SPEC.md 2.5 / 4.12).  RS: one more Philox block on
// counter stream 4 before the asset normals gives the step's regime s_t and the next step's; the row pair's chain runs on (mu, L) where the
// wave has a lane in regime 0 and then, under `if (s_t)`, on (mu1, L1) -- each a whole chain of its own, nothing shared (SPEC.md 2.6 / 4.13).  UHI: the same step with p_hi a scalar (philox4x32_10_uhi), the drift read through the LDS address
// par_lds instead of the opaque zero offset, the blocks scheduled one at a time, the factor's row pairs two at a time and the wave's
// priority raised over the factor (MCP_EXP_GEMV2, MCP_EXP_PRIO).  PI: the update of V is the floor rule of SPEC.md
// 4.15 on the step's rho, then the peak M.  SP (with CF): the flow is the path's own -w, and the step adds what it pays out to Y
// (SPEC.md 4.16); the reviews of w are events of the walk, not of the step.  LT (with CF): the mask that selects the step's V also
// adds one to the lifetime l (SPEC.md 4.17).  VT: the update of V is the targeting rule of SPEC.md 4.19 on the step's rho, then the
// variance estimate s moves on rho.  PU: the row pair's accumulator starts at the path's own drift pair m (SPEC.md 4.21), held in
// registers since before step 0, instead of the launch's mu; the drift is then not read from LDS.
      float rho[EM][KT];
      float fsh[PPT];                                  // FH: the shock s_j of the step's row (SPEC.md 2.4)
      if constexpr (BOOT) {
        // SPEC.md 2.1 / 4.4: one Philox block on counter (t, 1, p_lo, p_hi); j_t = mulhi(x0, R) on a restart (t = 0 or
        // x1 < thr), else the next row, circularly; rho_k = sum_i w_ki r_i, i ascending over N4 (zero-padded rows)
        asm volatile("" : "+s"(Wk));
        if constexpr (FH) asm volatile("" : "+s"(mu));   // the drift's scalar loads stay inside the step
#pragma unroll
        for (int e = 0; e < PPT; e++) {
          uint32_t x[4];
          philox4x32_10((uint32_t)t, 1u, plo[e], phi[e], ks, x);
          const uint32_t start = __umulhi(x[0], bt.n_rows);
          const uint32_t next = jrow[e] + 1u;
          jrow[e] = (t == 0 || (uint64_t)x[1] < bt.thr) ? start : (next == bt.n_rows ? 0u : next);
          const uint32_t j = jrow[e];
          float4 r4[NB];
          if constexpr (BLDS) {
            const uint32_t sw = BootSwizzle<NB>::of(j);
#pragma unroll
            for (int q = 0; q < NB; q++) r4[q] = s_tab[j * NB + ((uint32_t)q ^ sw)];
          } else {
            const float4* src = bt.rows + (size_t)j * NB;
#pragma unroll
            for (int q = 0; q < NB; q++) r4[q] = src[q];
          }
          if constexpr (FH) {
            // SPEC.md 4.11: sigma = sqrt(h) (IEEE, correctly rounded), r_i = fma(sigma, E_ji, mu_i) over N4 (zero-padded rows and drift)
            if constexpr (BLDS) fsh[e] = ((const float*)&s_tab[bt.n_rows * (uint32_t)NB])[j];
            else fsh[e] = fshock[j];
            const float sg = sqrtf(gh[e]);
#pragma unroll
            for (int q = 0; q < NB; q++) {
              r4[q].x = fma32(sg, r4[q].x, mu[4 * q + 0]);
              r4[q].y = fma32(sg, r4[q].y, mu[4 * q + 1]);
              r4[q].z = fma32(sg, r4[q].z, mu[4 * q + 2]);
              r4[q].w = fma32(sg, r4[q].w, mu[4 * q + 3]);
            }
          }
          if constexpr (REB) {
#pragma unroll
            for (int q = 0; q < NB; q++) {
              const f32x2 r0 = {r4[q].x, r4[q].y}, r1 = {r4[q].z, r4[q].w};
              const f32x2 a0 = Bs[e][2 * q] + r0, a1 = Bs[e][2 * q + 1] + r1;
              Bs[e][2 * q] = __builtin_elementwise_fma(Bs[e][2 * q], r0, a0);
              Bs[e][2 * q + 1] = __builtin_elementwise_fma(Bs[e][2 * q + 1], r1, a1);
            }
          } else {
#pragma unroll
          for (int k = 0; k < KT; k++) {
            float acc = 0.0f;
#pragma unroll
            for (int q = 0; q < NB; q++) {
              acc = fma32(Wk[k * N4 + 4 * q + 0], r4[q].x, acc);
              acc = fma32(Wk[k * N4 + 4 * q + 1], r4[q].y, acc);
              acc = fma32(Wk[k * N4 + 4 * q + 2], r4[q].z, acc);
              acc = fma32(Wk[k * N4 + 4 * q + 3], r4[q].w, acc);
            }
            rho[e][k] = acc;
          }
          }  // !REB
        }
      } else {
      // keep the (loop-invariant) parameter loads inside the step: hoisted, they would pin ~170 registers
      asm volatile("" : "+s"(mu), "+s"(Lp), "+s"(Wk));
      uint32_t par_off = 0;                                        // opaque zero: keeps the LDS reads inside the step too
      if constexpr (LDS_MU && !UHI) asm volatile("" : "+v"(par_off));
      const float* s_par = s_par0 + par_off;
      if constexpr (UHI) {                                         // the address itself, made opaque in place: no instruction
        asm volatile("" : "+v"(par_lds));
        s_par = (const float*)par_lds;
      }
      float jmp[PPT];                                  // JP: the step's market jump J of SPEC.md 2.5
      if constexpr (JP) {
        // SPEC.md 2.5: one Philox block on counter (t, 3, p_lo, p_hi); n = #{k : x0 < thr_k} (uint32 compares against wave-uniform
        // thresholds, scalar loads), g = Z(x1); J = fma(fl32(sqrt(nf) s32), g, fl32(nf m32)), the square root IEEE, correctly rounded.
        // Formed before the asset normals: only J stays live while they are.
        const cjump_p jk = jump_args(a);
        const float j_m = jk->m, j_s = jk->s;
#pragma unroll
        for (int e = 0; e < PPT; e++) {
          uint32_t x[4];
          philox4x32_10((uint32_t)t, 3u, plo[e], phi[e], ks, x);
          uint32_t n = 0u;
#pragma unroll
          for (int k = 0; k < 8; k++) n += x[0] < jk->thr[k] ? 1u : 0u;
          const float nf = (float)n;
          const float g = normal_icdf(x[1], s_tab, kc);
          jmp[e] = fma32(sqrtf(nf) * j_s, g, nf * j_m);
        }
      }
      bool rcur[PPT], rany0[PPT];                      // RS: is the step's regime s_t of SPEC.md 2.6 regime 1?  has the wave a lane in regime 0?
      if constexpr (RS) {
        // SPEC.md 2.6: one Philox block on counter (t, 4, p_lo, p_hi); s_0 = x1 < thr_start at t = 0, then s_{t+1} from x0 and the row
        // s_t of the transition matrix (uint64 compares against wave-uniform thresholds in [0, 2^32], scalar loads).  Formed before
        // the asset normals: only s_t and s_{t+1} stay live while they are.
        asm volatile("" : "+s"(mu1), "+s"(L1p));
        const cregime_p rk = regime_args(a);
        const uint64_t r01 = rk->thr01, r10 = rk->thr10, r_start = rk->thr_start;
#pragma unroll
        for (int e = 0; e < PPT; e++) {
          uint32_t x[4];
          philox4x32_10((uint32_t)t, 4u, plo[e], phi[e], ks, x);
          const uint32_t cur = t == 0 ? ((uint64_t)x[1] < r_start ? 1u : 0u) : rg[e];
          rg[e] = cur == 0u ? ((uint64_t)x[0] < r01 ? 1u : 0u) : ((uint64_t)x[0] < r10 ? 0u : 1u);
          rcur[e] = cur != 0u;
          rany0[e] = __ballot(cur == 0u) != 0ull;
        }
      }
      float z[PPT][N4];
      float st_s[PPT];                                 // STT: the step's scale s of SPEC.md 2.2 (GV: u of SPEC.md 4.9)
      if constexpr (STT) {
        // SPEC.md 2.2: chi = sum_k g_k^2 (fma, k = 4q + m ascending) over nt = ceil(nu/4) blocks on counter (t nt + q, 2, p_lo,
        // p_hi); the surplus words of the last block are masked to +0, which leaves chi unchanged.  nu is wave-uniform.
        const int dof = student_dof(a);
        if constexpr (GV) {                            // SPEC.md 4.9: nu = 0 is the Gaussian call, u = sigma = fl32(1 sigma)
#pragma unroll
          for (int e = 0; e < PPT; e++) st_s[e] = 1.0f;
        }
        if (!GV || dof != 0) {                         // wave-uniform
        const int nt = (dof + 3) >> 2;
        float chi[PPT];
#pragma unroll
        for (int e = 0; e < PPT; e++) chi[e] = 0.0f;
#pragma unroll 1
        for (int q = 0; q < nt; q++) {
          const uint32_t blk = (uint32_t)t * (uint32_t)nt + (uint32_t)q;   // T*nt < 2^32 (checked on the host)
          const int left = dof - 4 * q;                                   // words of this block that count (uniform)
#pragma unroll
          for (int e = 0; e < PPT; e++) {
            uint32_t x[4];
            float g[4];
            philox4x32_10(blk, 2u, plo[e], phi[e], ks, x);
            block_normals<false>(x, s_tab, kc, g[0], g[1], g[2], g[3]);
#pragma unroll
            for (int m = 0; m < 4; m++) {
              const float gm = m < left ? g[m] : 0.0f;
              chi[e] = fma32(gm, gm, chi[e]);
            }
          }
        }
        // s = sqrt(fl32(nu - 2) / max(chi, 2^-126)): IEEE division and square root, each correctly rounded
        const float num = (float)(dof - 2);
#pragma unroll
        for (int e = 0; e < PPT; e++) st_s[e] = sqrtf(num / fmaxf(chi[e], 0x1p-126f));
        }
        if constexpr (GV) {                            // u = fl32(s sigma), sigma = sqrt(h): IEEE, correctly rounded
#pragma unroll
          for (int e = 0; e < PPT; e++) st_s[e] = st_s[e] * sqrtf(gh[e]);
        }
      }
#pragma unroll
      for (int q = 0; q < NB; q++) {
        const uint32_t blk = (uint32_t)t * NB + q;     // counter.x; counter.y = 0 (T*NB < 2^32)
#pragma unroll
        for (int e = 0; e < PPT; e++) {
          uint32_t x[4];
          if constexpr (UHI) {
            // one block at a time: scheduled across the blocks, the step's temporaries pushed the values the epilogue needs to scratch
            __builtin_amdgcn_sched_barrier(0);
            philox4x32_10_uhi(blk, plo[e], uhi, ks, sk, x);
          } else {
            philox4x32_10(blk, 0u, plo[e], phi[e], ks, x);
          }
          block_normals<NATIVE, CEN>(x, s_tab, kc, z[e][0 * NB + q], z[e][1 * NB + q], z[e][2 * NB + q], z[e][3 * NB + q]);
          if constexpr (STT) {                         // SPEC.md 4.6: z' = fl32(s z)
#pragma unroll
            for (int m = 0; m < 4; m++) z[e][m * NB + q] = st_s[e] * z[e][m * NB + q];
          }
        }
      }
      if constexpr (GV) {
        // SPEC.md 4.9: q = sum_j z'_j^2 (fma, j ascending over the N assets; the padding normals j >= N masked to +0, which leaves
        // q unchanged), h = fminf(fma(b, h, fma(a_N, q, omega)), 2^40).  The constants are wave-uniform scalar loads.
        const cgarch_p gk = garch_args(a);
        const int n_live = gk->n_assets;
        const float g_an = gk->a_n, g_b = gk->b, g_om = gk->omega;
#pragma unroll
        for (int e = 0; e < PPT; e++) {
          float q = 0.0f;
#pragma unroll
          for (int j = 0; j < N4; j++) {
            const float zj = (j < N4 - 3 || j < n_live) ? z[e][j] : 0.0f;     // N > N4 - 4: only the last three can be padding
            q = fma32(zj, zj, q);
          }
          gh[e] = fminf(fma32(g_b, gh[e], fma32(g_an, q, g_om)), 0x1p40f);
        }
      }
      if constexpr (FOLD) {
        cfloat_p fv = mu + a.fold_offset;
        asm volatile("" : "+s"(fv));
#pragma unroll
        for (int e = 0; e < PPT; e++) {
          float acc = fv[0];
#pragma unroll
          for (int j = 0; j < N4; j++) acc = fma32(fv[1 + j], z[e][j], acc);
          rho[e][0] = acc;
        }
      } else {
      // r = mu + L z (row i: acc = mu_i, then j ascending), rho_k = sum_i w_ki r_i (i ascending)
#pragma unroll
      for (int e = 0; e < EM; e++)
#pragma unroll
        for (int k = 0; k < KT; k++) rho[e][k] = 0.0f;
      if constexpr (UHI && MCP_EXP_PRIO != 0) {
        // The lean kernel: the wave's priority is raised over the factor and the weight dot and dropped again behind the update of V
        // (two s_setprio per step), a hint to the instruction arbiter that changes no result: measured, not modelled
        // (profiles/gemv_feed_probe.json).  Nothing is scheduled across the boundary.
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
        __builtin_amdgcn_sched_barrier(0);
      }
      // Rows are processed in pairs (2m, 2m+1): one v_pk_fma_f32 per column does both rows, its L operand
      // an SGPR pair straight from the row-pair-interleaved parameter block, z_j broadcast by op_sel.
      if constexpr (UHI && MCP_EXP_GEMV2 != 0) {
        // The lean kernel: row pairs (m, m + 1) in flight together, m even (N4 / 2 = 2 NB is even), their two accumulators interleaved
        // column by column, so a packed fma is never followed by the one that reads its sum; row pair m + 1's two more columns finish
        // around row pair m's weights.  Every row keeps its own chain (mu_i, then j ascending) and rho its order (i ascending): the
        // same bits as the loop below.
#pragma unroll
        for (int m = 0; m < N4 / 2; m += 2) {
          f32x2 c0, c1;
          if constexpr (LDS_MU) { c0 = *(const f32x2*)&s_par[2 * m]; c1 = *(const f32x2*)&s_par[2 * m + 2]; }
          else { c0 = f32x2{mu[2 * m], mu[2 * m + 1]}; c1 = f32x2{mu[2 * m + 2], mu[2 * m + 3]}; }
          const int o0 = 2 * m * (m + 1), o1 = 2 * (m + 1) * (m + 2);       // the row pairs' offsets in the factor block
#pragma unroll
          for (int j = 0; j <= 2 * m + 1; j++) {
            const f32x2 l0 = {Lp[o0 + 2 * j], Lp[o0 + 2 * j + 1]}, l1 = {Lp[o1 + 2 * j], Lp[o1 + 2 * j + 1]};
            c0 = __builtin_elementwise_fma(l0, (f32x2){z[0][j], z[0][j]}, c0);
            c1 = __builtin_elementwise_fma(l1, (f32x2){z[0][j], z[0][j]}, c1);
          }
          const float w0 = LDS_W ? s_par[N4 + 2 * m] : Wk[2 * m], w1 = LDS_W ? s_par[N4 + 2 * m + 1] : Wk[2 * m + 1];
          const float w2 = LDS_W ? s_par[N4 + 2 * m + 2] : Wk[2 * m + 2], w3 = LDS_W ? s_par[N4 + 2 * m + 3] : Wk[2 * m + 3];
          {
            const int j = 2 * m + 2;
            const f32x2 l1 = {Lp[o1 + 2 * j], Lp[o1 + 2 * j + 1]};
            c1 = __builtin_elementwise_fma(l1, (f32x2){z[0][j], z[0][j]}, c1);
          }
          rho[0][0] = fma32(w0, c0.x, rho[0][0]);
          rho[0][0] = fma32(w1, c0.y, rho[0][0]);
          {
            const int j = 2 * m + 3;
            const f32x2 l1 = {Lp[o1 + 2 * j], Lp[o1 + 2 * j + 1]};
            c1 = __builtin_elementwise_fma(l1, (f32x2){z[0][j], z[0][j]}, c1);
          }
          rho[0][0] = fma32(w2, c1.x, rho[0][0]);
          rho[0][0] = fma32(w3, c1.y, rho[0][0]);
        }
      } else {
#pragma unroll
      for (int m = 0; m < N4 / 2; m++) {
        f32x2 acc[EM];
        if constexpr (RS) {
          // SPEC.md 4.13: row i is acc = mu^(s)_i, then fma(L^(s)_ij, z_j, acc), j ascending, s = s_t.  Two whole chains, each fed
          // as the plain kernel's (the factor an SGPR pair): regime 0's where the wave has a lane in regime 0 (a scalar branch; it
          // runs on every lane, those of regime 1 drop it), then regime 1's under the mask of its lanes, from mu1 -- never from the
          // other chain's sums -- skipped where no lane is in regime 1.  So a wave in one regime pays one chain.
#pragma unroll
          for (int e = 0; e < PPT; e++) {
            f32x2 c;
            if constexpr (LDS_MU) c = *(const f32x2*)&s_par[2 * m];
            else c = f32x2{mu[2 * m], mu[2 * m + 1]};
            if (rany0[e]) {
#pragma unroll
              for (int j = 0; j <= 2 * m + 1; j++) {
                const f32x2 l2 = {Lp[2 * m * (m + 1) + 2 * j], Lp[2 * m * (m + 1) + 2 * j + 1]};
                c = __builtin_elementwise_fma(l2, (f32x2){z[e][j], z[e][j]}, c);
              }
            }
            if (rcur[e]) {
              if constexpr (LDS_R) c = *(const f32x2*)&s_par[N4 + 2 * m];
              else c = f32x2{mu1[2 * m], mu1[2 * m + 1]};
#pragma unroll
              for (int j = 0; j <= 2 * m + 1; j++) {
                const f32x2 l2 = {L1p[2 * m * (m + 1) + 2 * j], L1p[2 * m * (m + 1) + 2 * j + 1]};
                c = __builtin_elementwise_fma(l2, (f32x2){z[e][j], z[e][j]}, c);
              }
            }
            acc[e] = c;
          }
        } else {
        f32x2 mu2;
        if constexpr (PU) mu2 = f32x2{0.0f, 0.0f};     // never read: the row pair starts from the path's own drift
        else if constexpr (LDS_MU) mu2 = *(const f32x2*)&s_par[2 * m];
        else mu2 = f32x2{mu[2 * m], mu[2 * m + 1]};
        if constexpr (PU) {                            // SPEC.md 4.21: acc = m, the pair the path drew before step 0
#pragma unroll
          for (int e = 0; e < PPT; e++) acc[e] = Dm[e][m];
        } else if constexpr (JP) {                            // SPEC.md 4.12: acc = fma(b_i, J, mu'_i), one packed fma per row pair
          f32x2 b2;
          if constexpr (LDS_B) {
            b2 = *(const f32x2*)&s_par[N4 + 2 * m];
          } else {
            const cfloat_p jb = (cfloat_p)jump_args(a)->loading;
            b2 = f32x2{jb[2 * m], jb[2 * m + 1]};
          }
#pragma unroll
          for (int e = 0; e < EM; e++) acc[e] = __builtin_elementwise_fma(b2, (f32x2){jmp[e % PPT], jmp[e % PPT]}, mu2);
        } else {
#pragma unroll
        for (int e = 0; e < EM; e++) acc[e] = mu2;
        }
#pragma unroll
        for (int j = 0; j <= 2 * m + 1; j++) {
          const f32x2 l2 = {Lp[2 * m * (m + 1) + 2 * j], Lp[2 * m * (m + 1) + 2 * j + 1]};   // (L[2m][j], L[2m+1][j])
#pragma unroll
          for (int e = 0; e < PPT; e++) acc[e] = __builtin_elementwise_fma(l2, (f32x2){z[e][j], z[e][j]}, acc[e]);
          if constexpr (ANTI) {                        // fma(L, -z, r): the negation is a source modifier of the packed fma
#pragma unroll
            for (int e = 0; e < PPT; e++) acc[PPT + e] = __builtin_elementwise_fma(l2, (f32x2){-z[e][j], -z[e][j]}, acc[PPT + e]);
          }
        }
        }  // !RS
        if constexpr (REB) {
#pragma unroll
          for (int e = 0; e < PPT; e++) {
            const f32x2 a2 = Bs[e][m] + acc[e];
            Bs[e][m] = __builtin_elementwise_fma(Bs[e][m], acc[e], a2);
          }
        } else {
        if constexpr (OV) {
          const auto ok = kernarg<PathArgsOV>();
          const uint32_t has = (uint32_t)(ok->ov.mask >> (2 * m)) & 3u;     // do the assets 2m, 2m+1 own rows?
          if (has) {
            typedef const __attribute__((address_space(4))) int32_t* cbeg_p;
            const cbeg_p rb = (cbeg_p)ok->ov.row_begin + 2 * m;
            const int b0 = rb[0], b1 = rb[1], b2 = rb[2];
            if (has & 1u) {
#pragma unroll
              for (int e = 0; e < PPT; e++) acc[e].x = overlay_return(acc[e].x, Ps[e][2 * m], b0, b1);
            }
            if (has & 2u) {
#pragma unroll
              for (int e = 0; e < PPT; e++) acc[e].y = overlay_return(acc[e].y, Ps[e][2 * m + 1], b1, b2);
            }
          }
        }
        if constexpr (AT) {
          const f32x2 w2 = {Wk[2 * m], Wk[2 * m + 1]};    // KT == 1: the pass's portfolio
#pragma unroll
          for (int e = 0; e < PPT; e++) At[e][m] = __builtin_elementwise_fma((f32x2){V[e][0], V[e][0]}, w2 * acc[e], At[e][m]);
        }
#pragma unroll
        for (int h = 0; h < 2; h++) {
          const int i = 2 * m + h;
#pragma unroll
          for (int k = 0; k < KT; k++) {
            const float wki = LDS_W ? s_par[N4 + i] : Wk[k * N4 + i];   // rows >= kt are zero-padded by pack_params
#pragma unroll
            for (int e = 0; e < EM; e++) rho[e][k] = fma32(wki, h ? acc[e].y : acc[e].x, rho[e][k]);
          }
        }
        }  // !REB
      }
      }  // !(UHI && GEMV2)
      }  // !FOLD
      }  // !BOOT
      if constexpr (SP) {
        // SPEC.md 4.16: U0 = fma(V, rho, V), U = U0 - w, live = V > 0 and U > 0; the step pays w, the step of ruin what is left of a
        // positive U0, every later step +0; V = live ? U : +0 -- a NaN U0 is ruin and pays +0.  No schedule is read.  V is +0 or
        // positive and w >= +0, always: at V = +0, U0 is +0 or NaN and U is not positive, so `U > 0` alone is `live`, and where the
        // path is not live fmaxf(U0, +0) is the payment in every case (IEEE maxNum: +0 for a NaN; a -0 adds nothing to Y >= +0).
        // One compare per value instead of three: the masks of eight portfolios would not fit the SGPRs beside the Cholesky factor.
#pragma unroll
        for (int e = 0; e < PPT; e++)
#pragma unroll
          for (int k = 0; k < KT; k++) {
            const float u0 = fma32(V[e][k], rho[e][k], V[e][k]);
            const float u = u0 - Wd[e][k];
            const bool lv = u > 0.0f;
            Yk[e][k] = Yk[e][k] + (lv ? Wd[e][k] : fmaxf(u0, 0.0f));
            V[e][k] = lv ? u : 0.0f;
            if constexpr (LT) Lk[e][k] += lv ? 1u : 0u;    // SPEC.md 4.17: the stored V is positive exactly where the path is live
          }
      } else if constexpr (CF) {
        // SPEC.md 4.7: U = fma(V, rho, V), U = U + c_s (two roundings), V = (V > 0 and U > 0) ? U : +0 -- a NaN U is ruin too
        const float cs = cash_flow(a, t);
#pragma unroll
        for (int e = 0; e < PPT; e++)
#pragma unroll
          for (int k = 0; k < KT; k++) {
            const float u = fma32(V[e][k], rho[e][k], V[e][k]) + cs;
            const bool lv = V[e][k] > 0.0f && u > 0.0f;
            V[e][k] = lv ? u : 0.0f;
            if constexpr (LT) Lk[e][k] += lv ? 1u : 0u;    // SPEC.md 4.17, on the mask of the select
          }
      } else if constexpr (PI) {
        // SPEC.md 4.15: F = fmaxf(S_t, fl32(theta M)), C = V - F, E = fmaxf(fminf(fl32(m C), fl32(b V)), +0), u = fma(V - E, rf, V),
        // V = fma(E, rho, u), M = fmaxf(M, V); fminf / fmaxf are IEEE minNum / maxNum.  S_t and the constants are wave-uniform
        // scalar loads inside the step.
        typedef const __attribute__((address_space(4))) float* cfloor_p;
        __builtin_amdgcn_sched_barrier(0);             // the rule's scalar loads stay behind the weight dot: issued earlier they are
                                                       // live across the step's SGPR peak and the compiler parks scalars in VGPR lanes
        const cprotect_p pk = protect_args(a);
        const float p_s = ((cfloor_p)pk->floor)[t], p_m = pk->m, p_b = pk->b, p_rf = pk->rf, p_th = pk->theta;
#pragma unroll
        for (int e = 0; e < PPT; e++)
#pragma unroll
          for (int k = 0; k < KT; k++) {
            const float fl = fmaxf(p_s, p_th * Mk[e][k]);
            const float ex = fmaxf(fminf(p_m * (V[e][k] - fl), p_b * V[e][k]), 0.0f);
            const float u = fma32(V[e][k] - ex, p_rf, V[e][k]);
            V[e][k] = fma32(ex, rho[e][k], u);
            Mk[e][k] = fmaxf(Mk[e][k], V[e][k]);
          }
      } else if constexpr (VT) {
        // SPEC.md 4.19: e = fminf(tgt / sqrtf(s), b), E = fl32(e V), u = fma(V - E, rf, V), U = fma(E, rho, u), D = fmaxf(E - V, +0),
        // U = fma(D, -sp, U), V = (V > 0 and U > 0) ? U : +0, Y = Y + e, s = fminf(fma(oml, fl32(rho rho), fl32(lam s)), 2^40).  The
        // square root and the division are IEEE, correctly rounded, one of each per path and portfolio; fminf / fmaxf are IEEE
        // minNum / maxNum (a NaN estimate becomes 2^40).  The constants are wave-uniform scalar loads inside the step.
        __builtin_amdgcn_sched_barrier(0);             // as the PI arm: the rule's scalar loads stay behind the weight dot
        const cvoltarget_p vk = vol_target_args(a);
        const float v_tgt = vk->tgt, v_lam = vk->lam, v_oml = vk->oml, v_b = vk->b, v_rf = vk->rf, v_sp = vk->sp;
#pragma unroll
        for (int e = 0; e < PPT; e++)
#pragma unroll
          for (int k = 0; k < KT; k++) {
            const float ee = fminf(v_tgt / sqrtf(Sg[e][k]), v_b);
            const float ex = ee * V[e][k];
            const float u = fma32(V[e][k] - ex, v_rf, V[e][k]);
            float uu = fma32(ex, rho[e][k], u);
            const float bor = fmaxf(ex - V[e][k], 0.0f);
            uu = fma32(bor, -v_sp, uu);
            V[e][k] = (V[e][k] > 0.0f && uu > 0.0f) ? uu : 0.0f;
            if constexpr (!DD) Yk[e][k] = Yk[e][k] + ee;
            Sg[e][k] = fminf(fma32(v_oml, rho[e][k] * rho[e][k], v_lam * Sg[e][k]), 0x1p40f);
          }
      } else if constexpr (!REB) {
#pragma unroll
      for (int e = 0; e < EM; e++)
#pragma unroll
        for (int k = 0; k < KT; k++)
          V[e][k] = logc ? (V[e][k] + rho[e][k]) : fma32(V[e][k], rho[e][k], V[e][k]);
      }
      if constexpr (UHI && MCP_EXP_PRIO != 0) __builtin_amdgcn_s_setprio(0);   // the step's other phase boundary
      if constexpr (FH) {
        // SPEC.md 4.11: d = fl32(h s_j), h = fminf(fma(b, h, fma(a, d, omega)), 2^40).  The constants are wave-uniform scalar loads.
        const cfilt_p fk = filt_args(a);
        const float f_a = fk->a, f_b = fk->b, f_om = fk->omega;
#pragma unroll
        for (int e = 0; e < PPT; e++) gh[e] = fminf(fma32(f_b, gh[e], fma32(f_a, gh[e] * fsh[e], f_om)), 0x1p40f);
      }
      if constexpr (DD) {
        // SPEC.md 4.2: P = fmax(P, V_t); q = fminf(q, V_t / P) (IEEE division) or d = fminf(d, S_t - P).  fminf is IEEE
        // minNum: the 0/0 of a zero peak is ignored.
#pragma unroll
        for (int e = 0; e < EM; e++)
#pragma unroll
          for (int k = 0; k < KT; k++) {
            Pk[e][k] = fmaxf(Pk[e][k], V[e][k]);
            Qk[e][k] = fminf(Qk[e][k], logc ? V[e][k] - Pk[e][k] : V[e][k] / Pk[e][k]);
            if constexpr (UW) {
              // SPEC.md 4.20: w = X_t < P against the peak just written (false on a NaN), c = w ? c + 1 : 0, m = max(m, c)
              Uc[e][k] = V[e][k] < Pk[e][k] ? Uc[e][k] + 1u : 0u;
              Um[e][k] = max(Um[e][k], Uc[e][k]);
            }
          }
      }
