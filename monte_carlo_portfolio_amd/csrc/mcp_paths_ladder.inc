// mcp_paths_ladder.inc -- every path kernel and the one selector (mcp_route.h: family, flag word) that runs it.  A selector runs
// the row it equals (mcp::selects) and no other; one without a row has no kernel.  Included where NB and KT are compile-time
// integers and MCP_ROW_IF(cond, family, mask, kernel) is defined: mcp_paths_inst.hip launches the kernel, host_selftest.cpp takes its
// name and proves that every request check_request accepts has exactly one row and that every row is reached.  `cond` states for
// which NB and KT the row exists; a row without one runs in passes of KT = 1 or 8 portfolios (PK_KT8).
#define MCP_ROW(family, mask, ...) MCP_ROW_IF(true, family, mask, __VA_ARGS__)

// The plain walk.  Gaussian draws compound either way, on the spec's normals or native math; one portfolio also on the folded
// step (rho = c + v.z) and, where the launch shares the high counter word (lean_range), on the lean step loop.
MCP_ROW(FAM_PLAIN, 0, mc_paths_kernel<NB, KT, 1, false, false, false>)
MCP_ROW(FAM_PLAIN, PK_LOGC, mc_paths_kernel<NB, KT, 1, false, false, true>)
MCP_ROW(FAM_PLAIN, PK_NATIVE, mc_paths_kernel<NB, KT, 1, true, false, false>)
MCP_ROW(FAM_PLAIN, PK_NATIVE | PK_LOGC, mc_paths_kernel<NB, KT, 1, true, false, true>)
MCP_ROW_IF(KT == 1, FAM_PLAIN, PK_FOLD, mc_paths_kernel<NB, 1, 1, false, true, false>)
MCP_ROW_IF(KT == 1, FAM_PLAIN, PK_FOLD | PK_LOGC, mc_paths_kernel<NB, 1, 1, false, true, true>)
MCP_ROW_IF(KT == 1 && NB <= LEAN_MAX_NB, FAM_PLAIN, PK_UHI, mc_paths_lean_kernel<NB, false>)
MCP_ROW_IF(KT == 1 && NB <= LEAN_MAX_NB, FAM_PLAIN, PK_UHI | PK_LOGC, mc_paths_lean_kernel<NB, true>)
MCP_ROW(FAM_PLAIN, PK_STT, mc_paths_t_kernel<NB, KT, 1>)
MCP_ROW(FAM_PLAIN, PK_GV, mc_paths_g_kernel<NB, KT, 1>)
MCP_ROW(FAM_PLAIN, PK_JP, mc_paths_j_kernel<NB, KT, 1>)
MCP_ROW(FAM_PLAIN, PK_RS, mc_paths_r_kernel<NB, KT, 1>)
MCP_ROW(FAM_PLAIN, PK_BOOT, mc_paths_boot_kernel<NB, KT, 1, false, false>)
MCP_ROW(FAM_PLAIN, PK_BOOT | PK_LOGC, mc_paths_boot_kernel<NB, KT, 1, true, false>)
MCP_ROW(FAM_PLAIN, PK_BOOT | PK_BLDS, mc_paths_boot_kernel<NB, KT, 1, false, true>)
MCP_ROW(FAM_PLAIN, PK_BOOT | PK_BLDS | PK_LOGC, mc_paths_boot_kernel<NB, KT, 1, true, true>)
MCP_ROW(FAM_PLAIN, PK_ANTI, mc_paths_anti_kernel<NB, KT, 1, false, PathArgsA>)
MCP_ROW(FAM_PLAIN, PK_ANTI | PK_LOGC, mc_paths_anti_kernel<NB, KT, 1, true, PathArgsA>)
MCP_ROW(FAM_PLAIN, PK_ANTI | PK_GV, mc_paths_anti_kernel<NB, KT, 1, false, PathArgsGA>)
// ... and on a drift drawn once per path (SPEC.md 2.7 / 4.21): the spec's normals and the unfolded recurrence, never the lean step loop
MCP_ROW(FAM_PLAIN, PK_PU, mc_paths_pu_kernel<NB, KT, 1, false>)
MCP_ROW(FAM_PLAIN, PK_PU | PK_LOGC, mc_paths_pu_kernel<NB, KT, 1, true>)

// The walk that tracks the drawdown
MCP_ROW(FAM_DD, 0, mc_paths_dd_kernel<NB, KT, 1, false>)
MCP_ROW(FAM_DD, PK_LOGC, mc_paths_dd_kernel<NB, KT, 1, true>)
MCP_ROW(FAM_DD, PK_STT, mc_paths_t_dd_kernel<NB, KT, 1>)
MCP_ROW(FAM_DD, PK_GV, mc_paths_g_dd_kernel<NB, KT, 1>)
MCP_ROW(FAM_DD, PK_JP, mc_paths_j_dd_kernel<NB, KT, 1>)
MCP_ROW(FAM_DD, PK_RS, mc_paths_r_dd_kernel<NB, KT, 1>)
MCP_ROW(FAM_DD, PK_ANTI, mc_paths_anti_kernel<NB, KT, 1, false, PathArgsADD>)
MCP_ROW(FAM_DD, PK_ANTI | PK_LOGC, mc_paths_anti_kernel<NB, KT, 1, true, PathArgsADD>)
MCP_ROW(FAM_DD, PK_ANTI | PK_GV, mc_paths_anti_kernel<NB, KT, 1, false, PathArgsGADD>)
MCP_ROW(FAM_DD, PK_PI | PK_GV, mc_paths_pi_kernel<NB, KT, 1, false, true>)
MCP_ROW(FAM_DD, PK_PI | PK_JP, mc_paths_pi_kernel<NB, KT, 1, true, true>)
MCP_ROW(FAM_DD, PK_VT | PK_GV, mc_paths_vt_kernel<NB, KT, 1, false, true>)
MCP_ROW(FAM_DD, PK_VT | PK_JP, mc_paths_vt_kernel<NB, KT, 1, true, true>)
// ... and the time under water (SPEC.md 4.20): the twins of the first two, of the GARCH walk (which also serves Student-t requests) and
// of the jump walk
MCP_ROW(FAM_DD, PK_UW, mc_paths_uw_kernel<NB, KT, 1, false>)
MCP_ROW(FAM_DD, PK_UW | PK_LOGC, mc_paths_uw_kernel<NB, KT, 1, true>)
MCP_ROW(FAM_DD, PK_UW | PK_GV, mc_paths_g_uw_kernel<NB, KT, 1>)
MCP_ROW(FAM_DD, PK_UW | PK_JP, mc_paths_j_uw_kernel<NB, KT, 1>)
// ... and the Gaussian drawdown walk on a drift drawn once per path (SPEC.md 4.21)
MCP_ROW(FAM_DD, PK_PU, mc_paths_pu_dd_kernel<NB, KT, 1, false>)
MCP_ROW(FAM_DD, PK_PU | PK_LOGC, mc_paths_pu_dd_kernel<NB, KT, 1, true>)

// The walk in segments between horizons.  The filtered rows, and the protection and the volatility target without a drawdown, run
// here with or without horizons (H = 0: one segment).
MCP_ROW(FAM_HZ, 0, mc_paths_hz_kernel<NB, KT, 1, false>)
MCP_ROW(FAM_HZ, PK_LOGC, mc_paths_hz_kernel<NB, KT, 1, true>)
MCP_ROW(FAM_HZ, PK_STT, mc_paths_t_hz_kernel<NB, KT, 1>)
MCP_ROW(FAM_HZ, PK_GV, mc_paths_g_hz_kernel<NB, KT, 1>)
MCP_ROW(FAM_HZ, PK_JP, mc_paths_j_hz_kernel<NB, KT, 1>)
MCP_ROW(FAM_HZ, PK_RS, mc_paths_r_hz_kernel<NB, KT, 1>)
MCP_ROW(FAM_HZ, PK_BOOT, mc_paths_boot_hz_kernel<NB, KT, 1, false, false>)
MCP_ROW(FAM_HZ, PK_BOOT | PK_LOGC, mc_paths_boot_hz_kernel<NB, KT, 1, true, false>)
MCP_ROW(FAM_HZ, PK_BOOT | PK_BLDS, mc_paths_boot_hz_kernel<NB, KT, 1, false, true>)
MCP_ROW(FAM_HZ, PK_BOOT | PK_BLDS | PK_LOGC, mc_paths_boot_hz_kernel<NB, KT, 1, true, true>)
MCP_ROW(FAM_HZ, PK_BOOT | PK_FH, mc_paths_fhs_kernel<NB, KT, 1, false>)
MCP_ROW(FAM_HZ, PK_BOOT | PK_FH | PK_BLDS, mc_paths_fhs_kernel<NB, KT, 1, true>)
MCP_ROW(FAM_HZ, PK_ANTI, mc_paths_anti_kernel<NB, KT, 1, false, PathArgsAHZ>)
MCP_ROW(FAM_HZ, PK_ANTI | PK_LOGC, mc_paths_anti_kernel<NB, KT, 1, true, PathArgsAHZ>)
MCP_ROW(FAM_HZ, PK_ANTI | PK_GV, mc_paths_anti_kernel<NB, KT, 1, false, PathArgsGAHZ>)
MCP_ROW(FAM_HZ, PK_PI | PK_GV, mc_paths_pi_kernel<NB, KT, 1, false, false>)
MCP_ROW(FAM_HZ, PK_PI | PK_JP, mc_paths_pi_kernel<NB, KT, 1, true, false>)
MCP_ROW(FAM_HZ, PK_VT | PK_GV, mc_paths_vt_kernel<NB, KT, 1, false, false>)
MCP_ROW(FAM_HZ, PK_VT | PK_JP, mc_paths_vt_kernel<NB, KT, 1, true, false>)
MCP_ROW(FAM_HZ, PK_PU, mc_paths_pu_hz_kernel<NB, KT, 1, false>)
MCP_ROW(FAM_HZ, PK_PU | PK_LOGC, mc_paths_pu_hz_kernel<NB, KT, 1, true>)

// Rebalancing on a period; within tolerance bands (SPEC.md 4.18) every portfolio is a pass of its own
MCP_ROW(FAM_REB, 0, mc_paths_reb_kernel<NB, KT, 1, false, false>)
MCP_ROW(FAM_REB, PK_BOOT, mc_paths_reb_kernel<NB, KT, 1, true, false>)
MCP_ROW(FAM_REB, PK_BOOT | PK_BLDS, mc_paths_reb_kernel<NB, KT, 1, true, true>)
MCP_ROW_IF(KT == 1, FAM_REB, PK_TB, mc_paths_band_kernel<NB, 1, 1, false, false>)
MCP_ROW_IF(KT == 1, FAM_REB, PK_TB | PK_BOOT, mc_paths_band_kernel<NB, 1, 1, true, false>)
MCP_ROW_IF(KT == 1, FAM_REB, PK_TB | PK_BOOT | PK_BLDS, mc_paths_band_kernel<NB, 1, 1, true, true>)

// Cash flows: the schedule, the path's own withdrawal (SPEC.md 4.16), the weights on a schedule (4.14), and the lifetime twins of
// the last two (4.17; the glide twin on G = 0 is the plain cash-flow walk with a lifetime)
MCP_ROW(FAM_CF, 0, mc_paths_cf_kernel<NB, KT, 1, false, false, false>)
MCP_ROW(FAM_CF, PK_STT, mc_paths_cf_kernel<NB, KT, 1, false, false, true>)
MCP_ROW(FAM_CF, PK_BOOT, mc_paths_cf_kernel<NB, KT, 1, true, false, false>)
MCP_ROW(FAM_CF, PK_BOOT | PK_BLDS, mc_paths_cf_kernel<NB, KT, 1, true, true, false>)
MCP_ROW(FAM_CF, PK_SP, mc_paths_spend_kernel<NB, KT, 1, false, false, false>)
MCP_ROW(FAM_CF, PK_SP | PK_STT, mc_paths_spend_kernel<NB, KT, 1, false, false, true>)
MCP_ROW(FAM_CF, PK_SP | PK_BOOT, mc_paths_spend_kernel<NB, KT, 1, true, false, false>)
MCP_ROW(FAM_CF, PK_SP | PK_BOOT | PK_BLDS, mc_paths_spend_kernel<NB, KT, 1, true, true, false>)
MCP_ROW(FAM_CF, PK_GP, mc_paths_glide_kernel<NB, KT, 1, false, false, false>)
MCP_ROW(FAM_CF, PK_GP | PK_STT, mc_paths_glide_kernel<NB, KT, 1, false, false, true>)
MCP_ROW(FAM_CF, PK_GP | PK_BOOT, mc_paths_glide_kernel<NB, KT, 1, true, false, false>)
MCP_ROW(FAM_CF, PK_GP | PK_BOOT | PK_BLDS, mc_paths_glide_kernel<NB, KT, 1, true, true, false>)
MCP_ROW(FAM_CF, PK_SP | PK_LT, mc_paths_spend_life_kernel<NB, KT, 1, false, false, false>)
MCP_ROW(FAM_CF, PK_SP | PK_LT | PK_STT, mc_paths_spend_life_kernel<NB, KT, 1, false, false, true>)
MCP_ROW(FAM_CF, PK_SP | PK_LT | PK_BOOT, mc_paths_spend_life_kernel<NB, KT, 1, true, false, false>)
MCP_ROW(FAM_CF, PK_SP | PK_LT | PK_BOOT | PK_BLDS, mc_paths_spend_life_kernel<NB, KT, 1, true, true, false>)
MCP_ROW(FAM_CF, PK_GP | PK_LT, mc_paths_glide_life_kernel<NB, KT, 1, false, false, false>)
MCP_ROW(FAM_CF, PK_GP | PK_LT | PK_STT, mc_paths_glide_life_kernel<NB, KT, 1, false, false, true>)
MCP_ROW(FAM_CF, PK_GP | PK_LT | PK_BOOT, mc_paths_glide_life_kernel<NB, KT, 1, true, false, false>)
MCP_ROW(FAM_CF, PK_GP | PK_LT | PK_BOOT | PK_BLDS, mc_paths_glide_life_kernel<NB, KT, 1, true, true, false>)
// ... and the Gaussian cash-flow walk on a drift drawn once per path (SPEC.md 4.21)
MCP_ROW(FAM_CF, PK_PU, mc_paths_pu_cf_kernel<NB, KT, 1>)

// The option overlay, with or without the drawdown
MCP_ROW(FAM_OV, 0, mc_paths_ov_kernel<NB, KT, 1, false, false>)
MCP_ROW(FAM_OV, PK_DD, mc_paths_ov_kernel<NB, KT, 1, false, true>)
MCP_ROW(FAM_OV, PK_STT, mc_paths_ov_kernel<NB, KT, 1, true, false>)
MCP_ROW(FAM_OV, PK_STT | PK_DD, mc_paths_ov_kernel<NB, KT, 1, true, true>)

// The attribution walk (SPEC.md 4.10): one portfolio per pass, the GARCH kernel's draws
MCP_ROW_IF(KT == 1, FAM_AT, PK_GV, mc_paths_attr_kernel<NB, 1, 1>)
#undef MCP_ROW
