// mcp_paths_body.inc -- the body of every path kernel of mcp_paths.h (they are listed there, each with the flags it sets); the
// step itself is mcp_paths_step.inc.  Included textually: as a shared __device__ function the plain kernel's registers came out
// allocated differently.  Every feature is an `if constexpr` on its flag, so a kernel without it keeps its code; without HZ the
// walk is the one loop it always was.  In scope: the template parameters NB, KT, PPT, the flags F (PathFlagsOff or a struct
// derived from it) and the kernel argument `a` (PathArgs or a struct that starts with one).
  constexpr bool NATIVE = F::NATIVE, FOLD = F::FOLD, LOGC = F::LOGC, DD = F::DD, HZ = F::HZ, BOOT = F::BOOT, BLDS = F::BLDS, REB = F::REB,
                 STT = F::STT, CF = F::CF, OV = F::OV, GV = F::GV, AT = F::AT, ANTI = F::ANTI, FH = F::FH, UHI = F::UHI, JP = F::JP, RS = F::RS,
                 GP = F::GP, PI = F::PI, SP = F::SP, LT = F::LT, TB = F::TB, VT = F::VT, UW = F::UW, PU = F::PU;
  static_assert(!UHI || (KT == 1 && PPT == 1 && !(NATIVE || FOLD || DD || HZ || BOOT || REB || STT || CF || OV || GV || AT || ANTI || FH || JP || RS || PI)),
                "uniform high counter word: the plain Gaussian walk of one portfolio only");
  static_assert(!FH || (BOOT && HZ && !(LOGC || REB || CF || STT || GV || OV || AT || DD || PI)), "filtered rows: the bootstrap's segmented walk only");
  static_assert(!JP || !(NATIVE || FOLD || LOGC || BOOT || REB || STT || CF || OV || GV || AT || ANTI || FH),
                "jump-diffusion: the Gaussian walk, its drawdown and its horizons, simple compounding only");
  static_assert(!RS || !(NATIVE || FOLD || LOGC || BOOT || REB || STT || CF || OV || GV || AT || ANTI || FH || JP || PI),
                "regime switching: the Gaussian walk, its drawdown and its horizons, simple compounding only");
  static_assert(!GP || (CF && HZ && !(NATIVE || FOLD || LOGC || DD || REB || OV || GV || AT || ANTI || FH || UHI || JP || RS || PI)),
                "glide path: the cash-flow kernel's segmented walk only");
  static_assert(!PI || (HZ && (JP || (STT && GV)) && !(NATIVE || FOLD || LOGC || BOOT || REB || CF || OV || AT || ANTI || FH || UHI || RS || GP)),
                "floor protection: the segmented GARCH or jump walk, simple compounding only");
  static_assert(!SP || (CF && HZ && !(NATIVE || FOLD || LOGC || DD || REB || OV || GV || AT || ANTI || FH || UHI || JP || RS || GP || PI)),
                "spending rule: the cash-flow kernel's segmented walk only");
  static_assert(!LT || (CF && (GP || SP)), "lifetime: the glide and spending kernels' walks only");
  static_assert(!TB || (REB && KT == 1), "tolerance bands: the rebalancing kernel's walk, one portfolio per pass");
  static_assert(!VT || (HZ && (JP || (STT && GV)) && !(NATIVE || FOLD || LOGC || BOOT || REB || CF || OV || AT || ANTI || FH || UHI || RS || GP || PI || SP || LT || TB)),
                "volatility targeting: the segmented GARCH or jump walk, simple compounding only");
  static_assert(!UW || (DD && !(NATIVE || FOLD || HZ || BOOT || REB || CF || OV || AT || ANTI || FH || UHI || RS || GP || PI || SP || LT || TB || VT)),
                "time under water: the drawdown walk on Gaussian draws, the GARCH walk or the jump walk only");
  static_assert(!PU || !(NATIVE || FOLD || UHI || BOOT || REB || STT || GV || OV || AT || ANTI || FH || JP || RS || GP || PI || SP || LT || TB || VT || UW),
                "drift uncertainty: the Gaussian walk, its drawdown, its horizons and its cash flows on the spec's normals only");
  constexpr int N4 = 4 * NB;
  // ANTI (SPEC.md 2.3): a lane's PPT draws feed EM = 2 PPT members -- slot e < PPT walks on z[e], slot PPT + e on -z[e]; p, live and
  // the counters are per draw (a.path_begin and a.n_paths count pairs), the members 2 p and 2 p + 1 are adjacent in the output rows
  constexpr int EM = ANTI ? 2 * PPT : PPT;
  static_assert(!ANTI || !(NATIVE || FOLD || BOOT || REB || CF || OV || AT || FH || PI), "antithetic pairs: the lean Gaussian and GARCH walks only");
  // wave-uniform parameters through the constant address space -> s_load_dword* into SGPRs
  typedef const __attribute__((address_space(4))) float* cfloat_p;
  cfloat_p mu = (cfloat_p)a.packed;
  cfloat_p Lp = mu + N4;
  cfloat_p Wk = mu + N4 + N4 * (N4 / 2 + 1) + (size_t)a.k_begin * N4;
  const int kt = min(KT, a.n_portfolios - a.k_begin);   // live portfolios in this pass (uniform)
  // inverse-CDF table: 16.5 KiB of LDS per block, filled once from the device-resident copy
  // CEN: the lean kernel's copy is scaled by each entry's binade as it is filled, for normal_icdf_centred (exact; once per workgroup,
  // nothing of it lives in the step loop)
  constexpr bool CEN = UHI && MCP_EXP_ICDF_CENTRED != 0;
  __shared__ float4 s_tab[ICDF_LDS_ENTRIES];
  if constexpr (CEN) {
    for (int i = threadIdx.x; i < ICDF_ENTRIES; i += PATH_BLOCK) s_tab[ICDF_PAD + i] = icdf_scaled_entry(a.tables[i], i);
  } else if constexpr (!NATIVE && !BOOT) {
    for (int i = threadIdx.x; i < ICDF_ENTRIES; i += PATH_BLOCK) s_tab[ICDF_PAD + i] = a.tables[i];
  }
  // BOOT: the observed rows (SPEC.md 2.1); BLDS: copied into the table's slot, chunk q of row j at j NB + (q ^ s(j))
  // (BootSwizzle), with ordinary vector LDS writes
  BootArgs bt{};
  if constexpr (BOOT) bt = boot_args(a);
  if constexpr (BOOT && BLDS) {
    for (uint32_t i = threadIdx.x; i < bt.n_rows * (uint32_t)NB; i += PATH_BLOCK) {
      const uint32_t j = i / NB, q = i % NB;
      s_tab[j * NB + (q ^ BootSwizzle<NB>::of(j))] = bt.rows[i];
    }
  }
  // FH: the rows' shocks (SPEC.md 2.4), [R] floats; BLDS: copied behind the rows, not swizzled (filt_fits_lds)
  const float* fshock = nullptr;
  if constexpr (FH) fshock = filt_args(a)->shock;
  if constexpr (FH && BLDS) {
    for (uint32_t i = threadIdx.x; i < (bt.n_rows + 3u) / 4u; i += PATH_BLOCK) s_tab[bt.n_rows * (uint32_t)NB + i] = ((const float4*)fshock)[i];
  }
  // The 512 B of padding in front of the table hold the drift (and, for one portfolio, the weights): read from LDS they
  // land in VGPRs without a VALU instruction (a v_mov from an SGPR costs an issue slot, an SGPR operand halves the
  // issue rate of the weight-dot FMAs).
  constexpr bool LDS_MU = MCP_EXP_LDSPAR >= 1 && !NATIVE && !FOLD && !BOOT;
  constexpr bool LDS_W = MCP_EXP_LDSPAR >= 2 && !NATIVE && !FOLD && !BOOT && KT == 1;
  float* const s_par0 = (float*)&s_tab[0];
  if constexpr (LDS_MU) {
    if (threadIdx.x < N4) { s_par0[threadIdx.x] = mu[threadIdx.x]; if (LDS_W) s_par0[N4 + threadIdx.x] = Wk[threadIdx.x]; }
  }
  // JP: the loadings b (SPEC.md 4.12) take the N4 floats behind the drift, the slot the weights of LDS_W would take
  constexpr bool LDS_B = JP && LDS_MU && !LDS_W;
  if constexpr (LDS_B) {
    if (threadIdx.x < N4) s_par0[N4 + threadIdx.x] = ((cfloat_p)jump_args(a)->loading)[threadIdx.x];
  }
  // RS: the drift of regime 1 (SPEC.md 4.13) takes the same N4 floats behind the drift; the factor of regime 1 follows it in the
  // regime block and is fed as the packed block's own, by scalar loads inside the step (no SGPR is held across steps for it)
  constexpr bool LDS_R = RS && LDS_MU && !LDS_W;
  cfloat_p mu1 = nullptr, L1p = nullptr;
  if constexpr (RS) {
    mu1 = (cfloat_p)regime_args(a)->block1;
    L1p = mu1 + N4;
  }
  if constexpr (LDS_R) {
    if (threadIdx.x < N4) s_par0[N4 + threadIdx.x] = mu1[threadIdx.x];
  }
  // statistics epilogue (N3): per-wave moment accumulators and the digit-0 histogram of one portfolio at a time
  __shared__ uint32_t s_hist[MCP_SELECT_BINS];
  __shared__ double s_mom[PATH_BLOCK / 64][KT][2];
  __shared__ float s_ext[PATH_BLOCK / 64][KT][2];
  __shared__ unsigned long long s_cnt[PATH_BLOCK / 64];
  // The epilogue's own arguments (pivot, partials, hist, slots, v0d: 13 dwords) are read from the kernel-argument segment
  // AFTER the step loop, through a pointer the compiler cannot see through: loaded up front they would sit in SGPRs for the
  // whole walk, and the kernel has none to spare (the Cholesky factor is fed from SGPRs): they spilled into VGPR lanes.  One
  // pointer, made opaque again in place before each use (not kernarg<PathArgs>() at each use: that moves every kernel's code).
  typedef const __attribute__((address_space(4))) PathArgs* cargs_p;
  cargs_p kargs = (cargs_p)__builtin_amdgcn_kernarg_segment_ptr();
  for (int i = threadIdx.x; i < MCP_SELECT_BINS; i += PATH_BLOCK) s_hist[i] = 0u;
  if (threadIdx.x < (PATH_BLOCK / 64) * KT) {
    (&s_mom[0][0][0])[2 * threadIdx.x] = 0.0; (&s_mom[0][0][0])[2 * threadIdx.x + 1] = 0.0;
    (&s_ext[0][0][0])[2 * threadIdx.x] = __builtin_inff(); (&s_ext[0][0][0])[2 * threadIdx.x + 1] = -__builtin_inff();
  }
  if (threadIdx.x < PATH_BLOCK / 64) s_cnt[threadIdx.x] = 0ull;
  if constexpr (AT) {                                      // the per-wave records of the attribution epilogue
    double* const s_at = attr_wave_slots<N4>();
    for (int i = threadIdx.x; i < (PATH_BLOCK / 64) * attr_record_len(N4); i += PATH_BLOCK) s_at[i] = 0.0;
  }
  if constexpr (ANTI) {                                    // the per-wave cross products of the pairs
    if (threadIdx.x < (PATH_BLOCK / 64) * KT) pair_wave_slots<KT>()[threadIdx.x] = 0.0;
  }
  __syncthreads();
  const auto kc = icdf_consts<UHI, CEN>();
  PhiloxKeys ks = philox_keys((uint32_t)a.seed, (uint32_t)(a.seed >> 32));
#if MCP_EXP_VKEYS
  // pin the 20 round keys in VGPRs: an SGPR operand halves the issue rate of the xor (profiles/r01_valu_rates.txt)
#pragma unroll
  for (int r = 0; r < 10; r++) { asm volatile("" : "+v"(ks.k0[r])); asm volatile("" : "+v"(ks.k1[r])); }
#endif
  // UHI: the scalar copies of the keys of rounds 1 to 3, the launch's p_hi, and the drift's LDS address in a VGPR of its own
  typedef const __attribute__((address_space(3))) float* lfloat_p;
  PhiloxUniformKeys sk{};
  uint32_t uhi = 0u;
  lfloat_p par_lds = nullptr;
  if constexpr (UHI) {
    sk = philox_uniform_keys((uint32_t)a.seed, (uint32_t)(a.seed >> 32));
    uhi = uniform_hi(a);
    par_lds = (lfloat_p)s_par0;
  }
  const int T = a.n_steps;
  constexpr bool logc = LOGC;

  const uint64_t tile = (uint64_t)PATH_BLOCK * PPT;
  const uint64_t n_tiles = (a.n_paths + tile - 1) / tile;
#ifdef MCP_DIAG_CLOCK
  const unsigned long long diag_t0 = __builtin_amdgcn_s_memtime(), diag_r0 = __builtin_amdgcn_s_memrealtime();
#endif
  for (uint64_t tl = blockIdx.x; tl < n_tiles; tl += gridDim.x) {
    uint64_t p[PPT];
    bool live[PPT];
    uint32_t plo[PPT], phi[PPT];
    float V[EM][KT];
    float Pk[EM][KT], Qk[EM][KT];                         // DD: running peak P and q (simple) / d (log)
    uint32_t jrow[PPT];                                   // BOOT: the row index j_t of SPEC.md 2.1
    f32x2 Bs[PPT][N4 / 2];                                // REB: the assets' returns since the last rebalance (SPEC.md 4.5)
    float Ps[PPT][N4];                                    // OV: the assets' price levels P_i (SPEC.md 4.8)
    float gh[PPT];                                        // GV, FH: the variance ratio h of SPEC.md 4.9 / 4.11
    f32x2 At[PPT][N4 / 2];                                // AT: the assets' contributions A_i of SPEC.md 4.10
    uint32_t rg[PPT];                                     // RS: the regime of the next step (SPEC.md 2.6); s_0 is drawn in step 0
    float Mk[EM][KT];                                     // PI: the running peak M of SPEC.md 4.15, V_0 included
    float Wd[PPT][KT], Yk[PPT][KT];                       // SP: the per-step withdrawal w and the total paid out Y of SPEC.md 4.16
    uint32_t Lk[PPT][KT];                                 // LT: the steps that stored a positive V, the lifetime l of SPEC.md 4.17
    uint32_t Tc[PPT];                                     // TB: the trade count c of SPEC.md 4.18
    float Ty[PPT];                                        // TB: the turnover Y of SPEC.md 4.18
    float Sg[PPT][KT];                                    // VT: the variance estimate s of SPEC.md 4.19; the summed exposure is Yk (!DD only)
    uint32_t Uc[PPT][KT], Um[PPT][KT];                    // UW: the current and the longest spell under water, c and m of SPEC.md 4.20
    f32x2 Dm[PPT][N4 / 2];                                // PU: the path's own drift m of SPEC.md 4.21, in the step's row pairs
#pragma unroll
    for (int e = 0; e < PPT; e++) {
      p[e] = tl * tile + (uint64_t)e * PATH_BLOCK + threadIdx.x;
      live[e] = p[e] < a.n_paths;
      const uint64_t g = a.path_begin + p[e];
      plo[e] = (uint32_t)g; phi[e] = (uint32_t)(g >> 32);
#pragma unroll
      for (int k = 0; k < KT; k++) V[e][k] = logc ? 0.0f : a.v0;
      if constexpr (PI) {
#pragma unroll
        for (int k = 0; k < KT; k++) Mk[e][k] = a.v0;
      }
      if constexpr (SP) {
        const float w0 = spend_args(a)->w0;               // one scalar load per tile
#pragma unroll
        for (int k = 0; k < KT; k++) { Wd[e][k] = w0; Yk[e][k] = 0.0f; }
      }
      if constexpr (LT) {
#pragma unroll
        for (int k = 0; k < KT; k++) Lk[e][k] = 0u;
      }
      if constexpr (VT) {                                 // s0_k of the pass's portfolios, scalar loads once per tile
        const cfloat_p s0 = (cfloat_p)vol_target_args(a)->s0 + a.k_begin;
#pragma unroll
        for (int k = 0; k < KT; k++) {
          Sg[e][k] = s0[k];
          if constexpr (!DD) Yk[e][k] = 0.0f;
        }
      }
      if constexpr (PU) {
        // SPEC.md 2.7 / 4.21: nb Philox blocks on counter (q, 5, p_lo, p_hi) give g, normal m of block q for asset m nb + q; then
        // m_i = mu_i and m_i = fma(M[i,j], g_j, m_i), j ascending -- the step's chain on M, row pairs by packed fma, the factor and the
        // drift scalar loads.  Per tile, so a second grid-stride tile draws its own; g and M die here, only m lives across the walk.
        const cfloat_p Mp = drift_factor(a);
        float g[N4];
#pragma unroll
        for (int q = 0; q < NB; q++) {
          uint32_t x[4];
          philox4x32_10((uint32_t)q, 5u, plo[e], phi[e], ks, x);
          block_normals<false>(x, s_tab, kc, g[0 * NB + q], g[1 * NB + q], g[2 * NB + q], g[3 * NB + q]);
        }
#pragma unroll
        for (int m = 0; m < N4 / 2; m++) {
          f32x2 c = f32x2{mu[2 * m], mu[2 * m + 1]};
#pragma unroll
          for (int j = 0; j <= 2 * m + 1; j++) {
            const f32x2 l2 = {Mp[2 * m * (m + 1) + 2 * j], Mp[2 * m * (m + 1) + 2 * j + 1]};   // (M[2m][j], M[2m+1][j])
            c = __builtin_elementwise_fma(l2, (f32x2){g[j], g[j]}, c);
          }
          Dm[e][m] = c;
        }
      }
      if constexpr (BOOT) jrow[e] = 0u;                   // replaced at t = 0 (a restart)
      if constexpr (GV) gh[e] = garch_args(a)->h0;        // one scalar load per tile
      if constexpr (FH) gh[e] = filt_args(a)->h0;
      if constexpr (RS) rg[e] = 0u;                       // replaced at t = 0
      if constexpr (REB) {
#pragma unroll
        for (int m = 0; m < N4 / 2; m++) Bs[e][m] = f32x2{0.0f, 0.0f};
      }
      if constexpr (TB) { Tc[e] = 0u; Ty[e] = 0.0f; }     // per tile, as B is: a second grid-stride tile starts from zero
      if constexpr (AT) {
#pragma unroll
        for (int m = 0; m < N4 / 2; m++) At[e][m] = f32x2{0.0f, 0.0f};
      }
      if constexpr (DD) {
#pragma unroll
        for (int k = 0; k < KT; k++) { Pk[e][k] = -__builtin_inff(); Qk[e][k] = logc ? 0.0f : 1.0f; }
      }
      if constexpr (UW) {
#pragma unroll
        for (int k = 0; k < KT; k++) { Uc[e][k] = 0u; Um[e][k] = 0u; }
      }
      if constexpr (OV) {                                 // P_i = fl32(spot_i), scalar loads once per tile
        typedef const __attribute__((address_space(4))) float* cspot_p;
        const cspot_p sp = (cspot_p)kernarg<PathArgsOV>()->ov.spot;
#pragma unroll
        for (int i = 0; i < N4; i++) Ps[e][i] = sp[i];
      }
      if constexpr (ANTI) {                               // the second member starts as the first
#pragma unroll
        for (int k = 0; k < KT; k++) {
          V[PPT + e][k] = V[e][k];
          if constexpr (DD) { Pk[PPT + e][k] = Pk[e][k]; Qk[PPT + e][k] = Qk[e][k]; }
        }
      }
    }

    if constexpr (REB) {
      // SPEC.md 4.5: the walk in segments that end at the events -- the next rebalance date nd, the next horizon, T.  Between
      // events the step updates B only.  At an event: the mark rho^_k = W_k.B (i ascending) and V^_k = fma(V_k, rho^_k, V_k),
      // the horizon store of V^, and at a date the trade (V_k = fma(V_k, rho'_k, V_k), B = +0) or, at T, V = V^.  The period,
      // cost and horizons are read where they are needed (kernarg), wave-uniform; every branch below is on wave-uniform values.
      int nd;                                              // the next rebalance date (s mod m == 0, s < T), T if none is left
      {
        const auto rs = kernarg<PathArgsRB>();
        const int per = rs->period;
        nd = (per >= 1 && per < T) ? per : T;
      }
      int t = 0, hi = 0;
      while (t < T) {
        const auto rs = kernarg<PathArgsRB>();
        const int t_hz = hi < rs->n_horizons ? rs->steps[hi] : T;
        const int t_end = min(nd, t_hz);
        for (; t < t_end; t++) {
#include "mcp_paths_step.inc"
        }
        float rh[PPT][KT], vh[PPT][KT];                    // rho^ and V^ at s = t
        asm volatile("" : "+s"(Wk));
#pragma unroll
        for (int e = 0; e < PPT; e++)
#pragma unroll
          for (int k = 0; k < KT; k++) {
            float acc = 0.0f;
#pragma unroll
            for (int m = 0; m < N4 / 2; m++) {
              acc = fma32(Wk[k * N4 + 2 * m], Bs[e][m].x, acc);
              acc = fma32(Wk[k * N4 + 2 * m + 1], Bs[e][m].y, acc);
            }
            rh[e][k] = acc;
            vh[e][k] = fma32(V[e][k], acc, V[e][k]);
          }
        const auto hs = kernarg<PathArgsRB>();
        if (hi < hs->n_horizons && hs->steps[hi] == t) {   // V_h of SPEC.md 4.3, before any trade of step h (t_hz may be T with no
                                                           // horizon left: the list is read again, nothing is stored then)
          float* const row = hs->hz + (size_t)(hi * a.n_portfolios + a.k_begin) * hs->hz_stride;
#pragma unroll
          for (int e = 0; e < PPT; e++)
            if (live[e]) {
#pragma unroll
              for (int k = 0; k < KT; k++)
                if (k < kt) row[(size_t)k * hs->hz_stride + p[e]] = vh[e][k];
            }
          hi++;
        }
        if (t == T) {
#pragma unroll
          for (int e = 0; e < PPT; e++)
#pragma unroll
            for (int k = 0; k < KT; k++) V[e][k] = vh[e][k];
        } else if constexpr (TB) {
          if (t == nd) {
            // SPEC.md 4.18: a review.  A lane trades when a watched asset is out of its band: |W_i| |B_i - rho^| >= tol_i (1 + rho^),
            // an IEEE compare (false on a NaN).  The mask bit and the tolerance are scalar loads, the test of the bit is wave-uniform, and an
            // unwatched asset forms no compare.  The trade is section 4.5's on the lanes that hit, by selects; a wave without a hit skips it.
            const cband_p bk = band_args(a);
            typedef const __attribute__((address_space(4))) uint32_t* cword_p;
            const cword_p wm = (cword_p)bk->watch + 2 * a.k_begin;
            const uint32_t w_lo = wm[0], w_hi = wm[1];
            cfloat_p tl = (cfloat_p)bk->tol + (size_t)a.k_begin * N4;
            bool hit[PPT];
#pragma unroll
            for (int e = 0; e < PPT; e++) hit[e] = false;
            asm volatile("" : "+s"(Wk));
#pragma unroll
            for (int i = 0; i < N4; i++) {
              if (((i < 32 ? w_lo : w_hi) >> (i & 31)) & 1u) {
                const float aw = fabsf(Wk[i]), tol = tl[i];
#pragma unroll
                for (int e = 0; e < PPT; e++) {
                  const float d = fabsf(((i & 1) ? Bs[e][i / 2].y : Bs[e][i / 2].x) - rh[e][0]);
                  const float x = aw * d;
                  const float g = fma32(tol, rh[e][0], tol);
                  hit[e] = hit[e] || x >= g;
                }
              }
            }
            unsigned long long any = 0ull;
#pragma unroll
            for (int e = 0; e < PPT; e++) any |= __ballot(hit[e]);
            if (any != 0ull) {                               // wave-uniform
              const float kap = kernarg<PathArgsTB>()->cost;
              asm volatile("" : "+s"(Wk));
#pragma unroll
              for (int e = 0; e < PPT; e++) {
                float tau = 0.0f;
#pragma unroll
                for (int m = 0; m < N4 / 2; m++) {
                  tau = fma32(fabsf(Wk[2 * m]), fabsf(Bs[e][m].x - rh[e][0]), tau);
                  tau = fma32(fabsf(Wk[2 * m + 1]), fabsf(Bs[e][m].y - rh[e][0]), tau);
                }
                const float rp = kap > 0.0f ? fma32(-kap, tau, rh[e][0]) : rh[e][0];
                const float vt = fma32(V[e][0], rp, V[e][0]);
                V[e][0] = hit[e] ? vt : V[e][0];
#pragma unroll
                for (int m = 0; m < N4 / 2; m++) {
                  Bs[e][m].x = hit[e] ? 0.0f : Bs[e][m].x;
                  Bs[e][m].y = hit[e] ? 0.0f : Bs[e][m].y;
                }
                Tc[e] += hit[e] ? 1u : 0u;
                Ty[e] = hit[e] ? Ty[e] + tau : Ty[e];
              }
            }
            const int per = kernarg<PathArgsTB>()->period;
            nd = per < T - t ? t + per : T;
          }
        } else if (t == nd) {                              // a rebalance date: the trade back to W
          const auto cs = kernarg<PathArgsRB>();
          const float kap = cs->cost;
          if (kap > 0.0f) {                                // rho' = rho^ - kappa tau, tau = sum_i |W_ki| |B_i - rho^_k|
            asm volatile("" : "+s"(Wk));
#pragma unroll
            for (int e = 0; e < PPT; e++)
#pragma unroll
              for (int k = 0; k < KT; k++) {
                float tau = 0.0f;
#pragma unroll
                for (int m = 0; m < N4 / 2; m++) {
                  tau = fma32(fabsf(Wk[k * N4 + 2 * m]), fabsf(Bs[e][m].x - rh[e][k]), tau);
                  tau = fma32(fabsf(Wk[k * N4 + 2 * m + 1]), fabsf(Bs[e][m].y - rh[e][k]), tau);
                }
                V[e][k] = fma32(V[e][k], fma32(-kap, tau, rh[e][k]), V[e][k]);
              }
          } else {
#pragma unroll
            for (int e = 0; e < PPT; e++)
#pragma unroll
              for (int k = 0; k < KT; k++) V[e][k] = vh[e][k];
          }
#pragma unroll
          for (int e = 0; e < PPT; e++)
#pragma unroll
            for (int m = 0; m < N4 / 2; m++) Bs[e][m] = f32x2{0.0f, 0.0f};
          const int per = cs->period;
          nd = per < T - t ? t + per : T;
        }
      }
    } else if constexpr (GP) {
      // SPEC.md 4.14: the walk in segments that end at the events -- the next horizon, the next break, T -- with the unchanged step
      // body.  At a horizon V_h is stored as below; at a break b_g the weight pointer moves to target block g for this pass, so step
      // b_g + 1 is the first on the new weights; both happen when they share a step.  Every tile starts on the packed weights again.
      // The horizons, the breaks and the targets are read where they are needed (kernarg), wave-uniform; every branch below is on
      // wave-uniform values.
      Wk = mu + N4 + N4 * (N4 / 2 + 1) + (size_t)a.k_begin * N4;
      int t = 0, hi = 0, gi = 0;
      while (t < T) {
        const auto gs = kernarg<PathArgsGP>();
        const int t_hz = hi < gs->n_horizons ? gs->steps[hi] : T;
        const int t_br = gi < gs->gp.n_breaks ? gs->gp.breaks[gi] : T;
        const int t_end = min(min(t_hz, t_br), T);
        for (; t < t_end; t++) {
#include "mcp_paths_step.inc"
        }
        const auto hs = kernarg<PathArgsGP>();
        if (hi < hs->n_horizons && hs->steps[hi] <= t) {   // V_h of SPEC.md 4.3, after the flow c_h (the host checked the lists: the
                                                           // step is t; `<=` so that every pass of the loop consumes an event or steps)
          float* const row = hs->hz + (size_t)(hi * a.n_portfolios + a.k_begin) * hs->hz_stride;
#pragma unroll
          for (int e = 0; e < PPT; e++)
            if (live[e]) {
#pragma unroll
              for (int k = 0; k < KT; k++)
                if (k < kt) row[(size_t)k * hs->hz_stride + p[e]] = V[e][k];
            }
          hi++;
        }
        if (gi < hs->gp.n_breaks && hs->gp.breaks[gi] <= t) {
          Wk = (cfloat_p)hs->gp.targets + (size_t)gi * hs->gp.stride + (size_t)a.k_begin * N4;
          gi++;
        }
      }
    } else if constexpr (SP) {
      // SPEC.md 4.16: the walk in segments that end at the events -- the next horizon, the next review nr, T -- with the step body
      // unchanged between them.  At a horizon V_h is stored as below; at a review (s mod every == 0, s < T: the review at T moves no
      // output) w' = fl32(w g32) and w = fminf(fmaxf(fl32(p32 V), fl32(w' lo32)), fl32(w' hi32)), on every lane -- a ruined path's w
      // is never paid; the store first when they share a step.  The period, the four constants and the horizons are read where they
      // are needed (kernarg), wave-uniform; every branch below is on wave-uniform values, and the next review is an addition.
      int nr;                                              // the next review (s mod every == 0, s < T), T if none is left
      {
        const int per = spend_args(a)->every;
        nr = (per >= 1 && per < T) ? per : T;
      }
      int t = 0, hi = 0;
      while (t < T) {
        const auto gs = kernarg<PathArgsSP>();
        const int t_hz = hi < gs->n_horizons ? gs->steps[hi] : T;
        const int t_end = min(min(t_hz, nr), T);
        for (; t < t_end; t++) {
#include "mcp_paths_step.inc"
        }
        const auto hs = kernarg<PathArgsSP>();
        if (hi < hs->n_horizons && hs->steps[hi] <= t) {   // V_h of SPEC.md 4.3, after the withdrawal of step h (the host checked the
                                                           // list: the step is t; `<=` so that every pass consumes an event or steps)
          float* const row = hs->hz + (size_t)(hi * a.n_portfolios + a.k_begin) * hs->hz_stride;
#pragma unroll
          for (int e = 0; e < PPT; e++)
            if (live[e]) {
#pragma unroll
              for (int k = 0; k < KT; k++)
                if (k < kt) row[(size_t)k * hs->hz_stride + p[e]] = V[e][k];
            }
          hi++;
        }
        if (t == nr && t < T) {                            // a review, after the store
          const cspend_p sk = spend_args(a);
          const float s_p = sk->p32, s_g = sk->g32, s_lo = sk->lo32, s_hi = sk->hi32;
#pragma unroll
          for (int e = 0; e < PPT; e++)
#pragma unroll
            for (int k = 0; k < KT; k++) {
              const float wp = Wd[e][k] * s_g;
              Wd[e][k] = fminf(fmaxf(s_p * V[e][k], wp * s_lo), wp * s_hi);
            }
          const int per = sk->every;
          nr = per < T - t ? t + per : T;
        }
      }
    } else if constexpr (HZ) {
      // SPEC.md 4.3: segment i runs the steps [h_{i-1}, h_i) with the unchanged step body and ends in one coalesced store
      // per live path and portfolio into row i*K + k of the horizon array; the last segment runs on to T.  The horizon
      // count, the steps and the array are read where they are needed, wave-uniform: the bounds through the plain kernel-argument
      // pointer (the compiler may place those loads), the array through kernarg.
      typedef const __attribute__((address_space(4))) PathArgsHZ* chz_p;
      chz_p hk = (chz_p)__builtin_amdgcn_kernarg_segment_ptr();
      const int n_seg = hk->n_horizons + 1;
      int t = 0;
      for (int seg = 0; seg < n_seg; seg++) {
        const int t_end = seg < n_seg - 1 ? hk->steps[seg] : T;
        for (; t < t_end; t++) {
#include "mcp_paths_step.inc"
        }
        if (seg < n_seg - 1) {                             // V_h (simple) / S_h (log) of SPEC.md 4.3
          const auto hs = kernarg<PathArgsHZ>();
          float* const row = hs->hz + (size_t)(seg * a.n_portfolios + a.k_begin) * hs->hz_stride;
#pragma unroll
          for (int e = 0; e < PPT; e++)
            if (live[e]) {
#pragma unroll
              for (int k = 0; k < KT; k++)
                if (k < kt) {
                  if constexpr (ANTI) *(float2*)&row[(size_t)k * hs->hz_stride + 2 * p[e]] = make_float2(V[e][k], V[PPT + e][k]);
                  else row[(size_t)k * hs->hz_stride + p[e]] = V[e][k];
                }
            }
        }
      }
    } else {
      for (int t = 0; t < T; t++) {
#include "mcp_paths_step.inc"
      }
    }

    if constexpr (AT) {
      // ---- attribution epilogue (SPEC.md 5.9): x, the tail flag x <= var (binary64), d = x - c; per asset the wave sums of A, of A
      // over the tail and of A d, added to this wave's record in LDS by lane 0 (its own slot: no race, fixed order over the tiles)
      const auto ak = &kernarg<PathArgsAT>()->at;
      asm volatile("" : "+s"(kargs));
      const double e_c = kargs->pivot[a.k_begin], e_var = ak->var[a.k_begin], e_v0d = kargs->v0d;
      int tid = threadIdx.x;
      asm volatile("" : "+v"(tid));                        // nothing derived from it (LDS addresses) is hoisted above the step loop
      const int lane = tid & 63, wv = tid >> 6;
      double* const slot = attr_wave_slots<N4>() + wv * attr_record_len(N4);
      double dv[PPT];
      bool tail[PPT];
      double cn = 0.0, ct = 0.0, s1 = 0.0;
#pragma unroll
      for (int e = 0; e < PPT; e++) {
        const double x = terminal_to_x(V[e][0], e_v0d, MCP_COMPOUND_SIMPLE);
        tail[e] = live[e] && x <= e_var;
        dv[e] = live[e] ? x - e_c : 0.0;
        cn += live[e] ? 1.0 : 0.0;                         // counts < 2^53: exact in double
        ct += tail[e] ? 1.0 : 0.0;
        s1 += dv[e];
      }
      cn = wave_sum(cn); ct = wave_sum(ct); s1 = wave_sum(s1);
      if (lane == 0) { slot[0] += cn; slot[1] += ct; slot[2] += s1; }
#pragma unroll
      for (int i = 0; i < N4; i++) {
        double sa = 0.0, st = 0.0, sx = 0.0;
#pragma unroll
        for (int e = 0; e < PPT; e++) {
          const double ai = live[e] ? (double)((i & 1) ? At[e][i / 2].y : At[e][i / 2].x) : 0.0;
          sa += ai;
          st += tail[e] ? ai : 0.0;
          sx = __builtin_fma(ai, dv[e], sx);
        }
        sa = wave_sum(sa); st = wave_sum(st); sx = wave_sum(sx);
        if (lane == 0) { slot[ATTR_HEAD + 3 * i] += sa; slot[ATTR_HEAD + 3 * i + 1] += st; slot[ATTR_HEAD + 3 * i + 2] += sx; }
      }
      float* const cb = ak->contrib;
      if (cb != nullptr) {                                 // wave-uniform: A_ki to [k][i][path], coalesced over the paths
        const int n_live = ak->n_assets;
        const uint64_t cs = ak->contrib_stride;
#pragma unroll
        for (int i = 0; i < N4; i++)
          if (i < n_live) {
#pragma unroll
            for (int e = 0; e < PPT; e++)
              if (live[e]) cb[((size_t)a.k_begin * n_live + i) * cs + p[e]] = (i & 1) ? At[e][i / 2].y : At[e][i / 2].x;
          }
      }
    } else {
#pragma unroll
    for (int e = 0; e < PPT; e++) {
      if (live[e]) {
#pragma unroll
        for (int k = 0; k < KT; k++)
          if (k < kt) {
            if constexpr (ANTI) *(float2*)&a.terminal[(size_t)(a.k_begin + k) * a.stride + 2 * p[e]] = make_float2(V[e][k], V[PPT + e][k]);
            else a.terminal[(size_t)(a.k_begin + k) * a.stride + p[e]] = V[e][k];
          }
        if constexpr (DD && OV) {                          // the drawdown output of the overlay kernel's arguments
          const auto dk = kernarg<PathArgsOV>();
#pragma unroll
          for (int k = 0; k < KT; k++)
            if (k < kt) dk->mdd[(size_t)(a.k_begin + k) * dk->mdd_stride + p[e]] = Qk[e][k];
        } else if constexpr (DD && PI) {                   // the drawdown output of the protection kernel's arguments
          const auto dk = kernarg<PathArgsPI>();
#pragma unroll
          for (int k = 0; k < KT; k++)
            if (k < kt) dk->mdd[(size_t)(a.k_begin + k) * dk->mdd_stride + p[e]] = Qk[e][k];
        } else if constexpr (DD && VT) {                   // the drawdown output of the targeting kernel's arguments
          const auto dk = kernarg<PathArgsPI>();
#pragma unroll
          for (int k = 0; k < KT; k++)
            if (k < kt) dk->mdd[(size_t)(a.k_begin + k) * dk->mdd_stride + p[e]] = Qk[e][k];
        } else if constexpr (VT) {                         // Y_T of SPEC.md 4.19, next to V_T
          const cvoltarget_p vk = vol_target_args(a);
#pragma unroll
          for (int k = 0; k < KT; k++)
            if (k < kt) vk->exposure[(size_t)(a.k_begin + k) * vk->exposure_stride + p[e]] = Yk[e][k];
        } else if constexpr (SP) {                         // Y_T of SPEC.md 4.16, next to V_T
          const cspend_p sk = spend_args(a);
#pragma unroll
          for (int k = 0; k < KT; k++)
            if (k < kt) sk->wd[(size_t)(a.k_begin + k) * sk->wd_stride + p[e]] = Yk[e][k];
        } else if constexpr (DD) {                         // the drawdown output, read from the kernel arguments here only
          const auto dk = kernarg<PathArgsDD>();
#pragma unroll
          for (int k = 0; k < KT; k++)
            if (k < kt) {
              if constexpr (ANTI) *(float2*)&dk->mdd[(size_t)(a.k_begin + k) * dk->mdd_stride + 2 * p[e]] = make_float2(Qk[e][k], Qk[PPT + e][k]);
              else dk->mdd[(size_t)(a.k_begin + k) * dk->mdd_stride + p[e]] = Qk[e][k];
            }
        }
        if constexpr (TB) {                                // c and Y of SPEC.md 4.18, next to V_T
          const cband_p bk = band_args(a);
          bk->trades[(size_t)a.k_begin * bk->trades_stride + p[e]] = Tc[e];
          bk->turnover[(size_t)a.k_begin * bk->turnover_stride + p[e]] = Ty[e];
        }
        if constexpr (UW) {                                // m and c_T of SPEC.md 4.20, next to V_T
          const cunderwater_p uk = underwater_args(a);
#pragma unroll
          for (int k = 0; k < KT; k++)
            if (k < kt) {
              uk->longest[(size_t)(a.k_begin + k) * uk->uw_stride + p[e]] = Um[e][k];
              uk->current[(size_t)(a.k_begin + k) * uk->uw_stride + p[e]] = Uc[e][k];
            }
        }
        if constexpr (LT) {                                // l of SPEC.md 4.17, next to V_T
          const clife_p lk = life_args(a);
#pragma unroll
          for (int k = 0; k < KT; k++)
            if (k < kt) lk->life[(size_t)(a.k_begin + k) * lk->life_stride + p[e]] = Lk[e][k];
        }
      }
    }
    }  // !AT

    // ---- fused statistics epilogue: V is still in registers ----
    asm volatile("" : "+s"(kargs));
    if (kargs->partials != nullptr) {                      // wave-uniform (kernel argument)
      const double* __restrict__ e_pivot = kargs->pivot;
      unsigned long long* __restrict__ e_hist = kargs->hist;
      const double e_v0d = kargs->v0d;
      int tid = threadIdx.x;
      asm volatile("" : "+v"(tid));                        // nothing derived from it (LDS addresses) is hoisted above the step loop
      const int lane = tid & 63, wv = tid >> 6;
      unsigned long long cnt = 0;
#pragma unroll
      for (int e = 0; e < PPT; e++) cnt += (unsigned long long)((EM / PPT) * __popcll(__ballot(live[e])));
      if (lane == 0) s_cnt[wv] += cnt;
#pragma unroll 1
      for (int k = 0; k < kt; k++) {
        const double c = e_pivot ? e_pivot[a.k_begin + k] : 0.0;
        double d1 = 0.0, d2 = 0.0;
        float mn = __builtin_inff(), mx = -__builtin_inff();
        double dm[EM];                                     // ANTI: d of every member, +0 for a dead lane
#pragma unroll
        for (int e = 0; e < EM; e++) {
          float v = V[e][0];
#pragma unroll
          for (int kk = 1; kk < KT; kk++) v = (kk == k) ? V[e][kk] : v;      // register select (k is a run-time index)
          if constexpr (ANTI) dm[e] = 0.0;
          if (live[e % PPT]) {
            const double d = terminal_to_x(v, e_v0d, logc ? MCP_COMPOUND_LOG : MCP_COMPOUND_SIMPLE) - c;
            d1 += d;
            d2 = __builtin_fma(d, d, d2);
            mn = fminf(mn, v);
            mx = fmaxf(mx, v);
            if constexpr (ANTI) dm[e] = d;
          }
          if (e_hist) lds_hist_add(s_hist, float_to_key(v) >> 21, live[e % PPT]);
        }
        d1 = wave_sum(d1); d2 = wave_sum(d2); mn = wave_minf(mn); mx = wave_maxf(mx);
        if (lane == 0) {                                   // this wave's own slot: no race, fixed order over the tiles
          s_mom[wv][k][0] += d1; s_mom[wv][k][1] += d2;
          s_ext[wv][k][0] = fminf(s_ext[wv][k][0], mn); s_ext[wv][k][1] = fmaxf(s_ext[wv][k][1], mx);
        }
        if constexpr (ANTI) {                              // SPEC.md 5.10: cross = sum (x_2j - c)(x_2j+1 - c), lane -> wave -> slot
          double cr = 0.0;
#pragma unroll
          for (int e = 0; e < PPT; e++) cr = __builtin_fma(dm[e], dm[PPT + e], cr);
          cr = wave_sum(cr);
          if (lane == 0) pair_wave_slots<KT>()[wv * KT + k] += cr;
        }
        if (e_hist) {                                      // flush portfolio k's digit-0 counts (read-and-clear)
          __syncthreads();
          unsigned long long* out = e_hist + (size_t)(a.k_begin + k) * 2 * MCP_SELECT_BINS;
          for (int i = tid; i < MCP_SELECT_BINS; i += PATH_BLOCK) {
            const uint32_t h = s_hist[i];
            if (h) { atomicAdd(&out[i], (unsigned long long)h); s_hist[i] = 0u; }
          }
          __syncthreads();
        }
      }
    }
  }

#ifdef MCP_DIAG_CLOCK
  if (threadIdx.x == 0 && blockIdx.x < 8192) {
    mcp_diag_stamps[2 * blockIdx.x] = __builtin_amdgcn_s_memtime() - diag_t0;
    mcp_diag_stamps[2 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime() - diag_r0;
  }
#endif
  asm volatile("" : "+s"(kargs));
  if (kargs->partials != nullptr) {
    __syncthreads();
    if ((int)threadIdx.x < kt) {                           // one partial per workgroup and portfolio, waves in order
      const int k = threadIdx.x;
      MomentPartial o;
      o.s1 = (s_mom[0][k][0] + s_mom[1][k][0]) + (s_mom[2][k][0] + s_mom[3][k][0]);
      o.s2 = (s_mom[0][k][1] + s_mom[1][k][1]) + (s_mom[2][k][1] + s_mom[3][k][1]);
      o.vmin = fminf(fminf(s_ext[0][k][0], s_ext[1][k][0]), fminf(s_ext[2][k][0], s_ext[3][k][0]));
      o.vmax = fmaxf(fmaxf(s_ext[0][k][1], s_ext[1][k][1]), fmaxf(s_ext[2][k][1], s_ext[3][k][1]));
      o.n = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
      kargs->partials[(size_t)(a.k_begin + k) * kargs->slots + blockIdx.x] = o;
      if constexpr (ANTI) {                                // one cross partial per workgroup and portfolio, waves in order
        const double* const s_cr = pair_wave_slots<KT>();
        pair_cross(a)[(size_t)(a.k_begin + k) * gridDim.x + blockIdx.x] = (s_cr[k] + s_cr[KT + k]) + (s_cr[2 * KT + k] + s_cr[3 * KT + k]);
      }
    }
  }
  if constexpr (AT) {
    // one record per workgroup: entry j is the sum of the four waves' entries j, waves in order (SPEC.md 5.9)
    __syncthreads();
    const auto ak = &kernarg<PathArgsAT>()->at;
    const double* const s_at = attr_wave_slots<N4>();
    constexpr int RL = attr_record_len(N4);
    if ((int)threadIdx.x < RL) {
      const int j = threadIdx.x;
      ak->partials[((size_t)a.k_begin * gridDim.x + blockIdx.x) * RL + j] = (s_at[j] + s_at[RL + j]) + (s_at[2 * RL + j] + s_at[3 * RL + j]);
    }
  }
