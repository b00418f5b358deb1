// What the 128-wide fused PPO / A2C update (k_ppo_wide.hip) and the folds behind it (k_ppo.hip) agree on.
#pragma once
#include "trl_head.h"

#define PPO_WIDE_H 128                              // the width the weight-stationary gradient kernel is built for
#define PPO_WIDE_S 32                               // samples of a workgroup's tile (k_ppo_wide.hip: why not 64)
// `ln_mask` value by which the host-side fold launchers of k_ppo.hip are told that the rows are a 128-wide pair's: neither
// LayerNorm bit is set, so the block lengths are the plain ones at H = 128
#define PPO_WIDE_MASK 8
// the fold / clip / Adam launch of a wide pair: ~360 jobs of 64 parameters per network run as a job loop on a grid that is
// always co-resident (one 8-wave block per CU of the smallest gfx950 part; two fit a CU at the kernel's 128-register bound)
#define PPO_WIDE_FOLD_BLOCKS 256

static inline bool ppo_wide_ok(int head, int D, int H, int A, int act) {
  return head >= HEAD_GAUSS && head <= HEAD_SD && H == PPO_WIDE_H && D >= 2 && D <= 32 && A >= HEADS[head].a_min &&
         A <= HEADS[head].a_max && (act == TRL_ACT_TANH || act == TRL_ACT_RELU);
}
