// wab_default_rules.h — the default options' rule fields of the parameter block as constants.
//
// The values wab_create resolves from the default options (include/wab.h's field comments,
// wab_gym_amd/options.py) on a batched surface with autoreset.  The small kernel's default-rules
// instances (wab_step_small<8, 11, .., RULES = true>) assign them to each wave's copy of the
// parameter block (specialise_rules), so that the fields' scalar loads, the registers that hold
// them and the branches on them fold away.  A handle takes those instances only when its own
// resolved fields equal the resolved default's (wab_capi.hip default_rules), never by comparison
// with this file: a wrong constant here fails the default options' parity tests.
#pragma once

#include "wab_params.h"

namespace wab {

struct DefaultRules {
  static constexpr int32_t n_actions = 5;  // lookout_only: four moves and "look out"
  static constexpr int32_t act_role4 = 0, act_role5 = -1;
  // wolf_chance_to_despawn 0.05: floor(0.05 * 2^53) + 1
  static constexpr uint32_t keep_th = 0x0CCCCCCCu, keep_tl = 0x19999Au;
  // T_1 of bush_power 100, max_berries_per_bush 200
  static constexpr uint32_t bush_th = 0xF11CBFADu, bush_tl = 0x314FCu;
  // chance_wolf_on_square 0.001: q = ceil(0.0005 * 2^53) 2^-53, gap[g] = floor((1 - q)^g 2^53)
  static constexpr float gap_inv_l2 = -0x1.5a7ca8p+10f;  // 1 / log2(1 - q)
  static constexpr uint32_t gap_full_th = 0xF0201C9Cu, gap_full_tl = 0x8E362u;   // gap[128]
  static constexpr uint32_t gap_ring_th = 0xF9ED79EBu, gap_ring_tl = 0x1EA280u;  // gap[48]
  static constexpr uint32_t gap_view_th = 0xF0F7B1F2u, gap_view_tl = 0x62973u;   // gap[121]
  static constexpr int32_t max_berries = 200;
  static constexpr float bush_power = 100.0f;
  static constexpr double fill = 1.0 / 8.0, hunger = 1.0 / 40.0;
  static constexpr double r_turn = 0.0, r_killed = -1.0, r_starve = -1.0, r_finish = 1.0, r_eat = 0.1;
  static constexpr double start_food = 1.0;
  static constexpr int32_t start_role = 1, start_food_random = 0, start_role_random = 0;
  static constexpr int32_t max_turns = 80, turns_empty = 40;
  static constexpr int32_t lookout_only = 1, restrict_view = 0, wolves_on = 1, wolves_can_move = 1, god_mode = 0,
                           autoreset = 1;
  static constexpr int32_t eaten_cap = 80;  // eaten_capacity 0: max_turns
};

template <bool RULES>
__host__ __device__ inline void specialise_rules(Params& p) {
  if constexpr (RULES) {
    using D = DefaultRules;
    p.n_actions = D::n_actions;
    for (int a = 0; a < 4; ++a) p.act_role[a] = -1;
    p.act_role[4] = D::act_role4; p.act_role[5] = D::act_role5;
    p.keep_th = D::keep_th; p.keep_tl = D::keep_tl;
    p.bush_th = D::bush_th; p.bush_tl = D::bush_tl;
    p.n_gap = kGapChunk;
    p.gap_inv_l2 = D::gap_inv_l2;
    p.gap_full_th = D::gap_full_th; p.gap_full_tl = D::gap_full_tl;
    p.gap_ring_th = D::gap_ring_th; p.gap_ring_tl = D::gap_ring_tl;
    p.gap_view_th = D::gap_view_th; p.gap_view_tl = D::gap_view_tl;
    p.max_berries = D::max_berries;
    p.bush_power = D::bush_power;
    p.fill = D::fill; p.hunger = D::hunger;
    p.r_turn = D::r_turn; p.r_killed = D::r_killed; p.r_starve = D::r_starve; p.r_finish = D::r_finish;
    p.r_eat = D::r_eat;
    p.start_food = D::start_food;
    p.start_role = D::start_role; p.start_food_random = D::start_food_random;
    p.start_role_random = D::start_role_random;
    p.max_turns = D::max_turns; p.turns_empty = D::turns_empty;
    p.lookout_only = D::lookout_only; p.restrict_view = D::restrict_view; p.wolves_on = D::wolves_on;
    p.wolves_can_move = D::wolves_can_move; p.god_mode = D::god_mode; p.autoreset = D::autoreset;
    p.eaten_cap = D::eaten_cap;
    p.wolf_cap = 8;  // (the instances are the 8-slot ones)
    // the view masks by role (wab_env.py:109-139, 0 lookout, 1 gatherer): 11-bit rows, and as
    // 121-bit planes (bit i*11 + j)
    { const uint32_t rows[11] = {0x707u, 0x603u, 0x401u, 0x000u, 0x000u, 0x000u, 0x000u, 0x000u, 0x401u, 0x603u, 0x707u};
      const uint32_t plane[4] = {0x00701F07u, 0x00000001u, 0x01000000u, 0x01C1F01Cu};
      for (int i = 0; i < 11; ++i) p.mask_rows[0][i] = rows[i];
      for (int k = 0; k < 4; ++k) p.view121[0][k] = plane[k]; }
    { const uint32_t rows[11] = {0x7FFu, 0x7FFu, 0x7FFu, 0x78Fu, 0x707u, 0x707u, 0x707u, 0x78Fu, 0x7FFu, 0x7FFu, 0x7FFu};
      const uint32_t plane[4] = {0xFFFFFFFFu, 0x83F07F1Fu, 0xFFF1FC1Fu, 0x01FFFFFFu};
      for (int i = 0; i < 11; ++i) p.mask_rows[1][i] = rows[i];
      for (int k = 0; k < 4; ++k) p.view121[1][k] = plane[k]; }
  }
}

}  // namespace wab
