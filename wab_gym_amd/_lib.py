"""ctypes binding of the C-ABI in include/wab.h (libwab_hip.so, built in-tree).

There is no fallback: if the HIP library is missing or fails to load, every product
entry point raises.  torch is imported first so that its bundled HIP runtime
(SONAME libamdhip64.so.7) is the one the library binds to — one runtime per process.
"""
from __future__ import annotations

import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("WAB_LIB") or os.path.join(HERE, "_lib", "libwab_hip.so")

EXPORTED = [
    "wab_abi_version", "wab_last_error", "wab_num_actions", "wab_create", "wab_destroy",
    "wab_reset", "wab_step", "wab_rollout", "wab_get_counters", "wab_get_state", "wab_batch",
    "wab_feature_dim", "wab_featurize", "wab_discounted_returns", "wab_step_kernel",
    "wab_superbasic_dim", "wab_featurize_superbasic", "wab_render", "wab_egocentric",
    "wab_debug_bush_values", "wab_step_features", "wab_discounted_returns_exact",
    "wab_bush_thresholds", "wab_rollout_features", "wab_render_envs", "wab_set_obs_placement",
    "wab_snapshot_bytes", "wab_snapshot_hash", "wab_snapshot_save", "wab_snapshot_restore",
    "wab_policy_create", "wab_policy_load", "wab_policy_act", "wab_policy_destroy",
    "wab_rollout_policy", "wab_rollout_policy_fused", "wab_debug_returns_plan", "wab_debug_policy_plan",
    "wab_episode_stats_workspace", "wab_episode_stats_update", "wab_normalize_episode_returns",
    "wab_gae", "wab_whiten_workspace", "wab_whiten", "wab_debug_gae_plan",
    "wab_policy_grad_workspace", "wab_policy_grad", "wab_policy_grad_bad_actions", "wab_debug_policy_grad_plan",
    "wab_policy_grad_ppo", "wab_policy_evaluate",
    "wab_policy_grad_gather", "wab_policy_grad_ppo_gather", "wab_policy_evaluate_gather", "wab_policy_grad_bad_rows",
    "wab_policy_adam_workspace", "wab_policy_adam_step",
    # WAB_HAS_PACKED_FEATURES: feature rows as 1 bit per feature
    "wab_feature_bits_pitch", "wab_features_pack", "wab_features_unpack", "wab_policy_evaluate_packed",
    "wab_policy_grad_packed", "wab_policy_grad_ppo_packed", "wab_rollout_policy_packed",
    # WAB_HAS_ACTION_RULE: greedy and temperature action selection
    "wab_policy_set_action_rule", "wab_policy_get_action_rule",
    # include/wab_torus.h: the Environment 2.0 torus world
    "wab2_abi_version", "wab2_last_error", "wab2_record_size", "wab2_create", "wab2_destroy",
    "wab2_batch", "wab2_reset", "wab2_step", "wab2_rollout", "wab2_get_state", "wab2_get_counters",
    "wab2_get_obs", "wab2_take_action", "wab2_create_at", "wab2_reset_at",
]

ABI2_VERSION = 1
OBS_SAME_BUFFER, OBS_FRESH_BUFFER = 0, 1  # wab_set_obs_placement

ABI_VERSION = 14
SNAPSHOT_MAGIC, SNAPSHOT_VERSION = 0x53424157, 1  # 'WABS' (wab_snapshot_info)


class WabObs(ctypes.Structure):
    _fields_ = [("planes", ctypes.c_void_p), ("food_turns", ctypes.c_void_p),
                ("role", ctypes.c_void_p), ("status", ctypes.c_void_p)]


class WabCounters(ctypes.Structure):
    _fields_ = [("wolf_overflow", ctypes.c_uint64), ("eaten_overflow", ctypes.c_uint64),
                ("bad_actions", ctypes.c_uint64), ("steps", ctypes.c_uint64),
                ("resets", ctypes.c_uint64), ("ego_missing", ctypes.c_uint64),
                ("handoff_timeouts", ctypes.c_uint64), ("wolf_overflow_reset", ctypes.c_uint64),
                ("rollout_launches", ctypes.c_uint64), ("rollout_step_calls", ctypes.c_uint64)]


class WabSnapshotInfo(ctypes.Structure):
    _fields_ = [("magic", ctypes.c_uint32), ("version", ctypes.c_uint32),
                ("config_hash", ctypes.c_uint64), ("seed", ctypes.c_uint64),
                ("env_id_first", ctypes.c_int64), ("count", ctypes.c_int64),
                ("record_bytes", ctypes.c_int64)]


class WabPolicyShape(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("in_features", "h1", "h2", "h3", "n_actions")]


class WabPolicyWeights(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("w1", "b1", "w2", "b2", "w3", "b3", "wa", "ba", "wv", "bv")]


VALUE_LOSS = {"smooth_l1": 0, "mse": 1}  # WAB_VALUE_LOSS_*
ACTION_MODE = {"sample": 0, "greedy": 1}  # WAB_ACT_*


class WabActionRule(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_int32), ("temperature", ctypes.c_float)]


class WabPpoConfig(ctypes.Structure):
    _fields_ = [("clip", ctypes.c_float), ("value_clip", ctypes.c_float)]


class WabPolicyLoss(ctypes.Structure):
    _fields_ = [("value_coef", ctypes.c_float), ("entropy_coef", ctypes.c_float), ("value_loss", ctypes.c_int32),
                ("scale", ctypes.c_float), ("accumulate", ctypes.c_int32), ("chunk_rows", ctypes.c_int32)]


class WabAdamConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_double) for n in ("lr", "beta1", "beta2", "eps", "weight_decay", "max_grad_norm")] \
        + [("decoupled", ctypes.c_int32)]


class WabAdamState(ctypes.Structure):  # device memory; this mirror reads a copy of it
    _fields_ = [("step", ctypes.c_uint64), ("skipped", ctypes.c_uint64), ("beta1_pow", ctypes.c_double),
                ("beta2_pow", ctypes.c_double), ("grad_norm", ctypes.c_float), ("clip_scale", ctypes.c_float),
                ("reserved", ctypes.c_uint64)]


class WabError(RuntimeError):
    pass


_lib = None


def load():
    """Load libwab_hip.so (raises if it is absent: build it with __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise WabError("libwab_hip.so not built (%s); run `python -c 'import __graft_entry__ as g; "
                       "g.build()'`" % LIB_PATH)
    try:
        import torch  # noqa: F401  (bind to torch's HIP runtime if torch is used)
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    if hasattr(L, "wab_diagnostic_build") and os.environ.get("WAB_DIAGNOSTIC_OK") != "1":
        # a stamps / store-floor / ablation build (csrc/wab_build_guard.h): results wrong by design
        raise WabError("%s is a diagnostic build (wab_diagnostic_build); the product library is "
                       "wab_gym_amd/_lib/libwab_hip.so (set WAB_DIAGNOSTIC_OK=1 only in tools/)" % LIB_PATH)
    P, I64, U64, I32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_int32
    L.wab_last_error.restype = ctypes.c_char_p
    L.wab_num_actions.argtypes = [P]
    L.wab_create.argtypes = [P, I64, U64, I64, ctypes.c_int, ctypes.POINTER(P)]
    L.wab_destroy.argtypes = [P]
    L.wab_reset.argtypes = [P, P, P, P]
    L.wab_step.argtypes = [P, P, P, P, P, P, P]
    L.wab_rollout.argtypes = [P, P, I32, P, P, P, P]
    L.wab_get_counters.argtypes = [P, P, P]
    L.wab_get_state.argtypes = [P, P, P, P, P, P, P, P]
    L.wab_feature_dim.argtypes = [P]
    L.wab_featurize.argtypes = [P, P, P, P, P]
    L.wab_superbasic_dim.argtypes = [P]
    L.wab_featurize_superbasic.argtypes = [P, P, P, P]
    L.wab_step_features.argtypes = [P, P, P, P, P, P, P]
    L.wab_render.argtypes = [P, P, I32, I32, P, P]
    L.wab_render_envs.argtypes = [P, P, I64, I64, I32, I32, P, P]
    L.wab_egocentric.argtypes = [P, P, P, P]
    L.wab_debug_bush_values.argtypes = [P, P, P, I64, P]
    L.wab_discounted_returns.argtypes = [P, P, I32, I64, ctypes.c_double, P, P, P]
    L.wab_discounted_returns_exact.argtypes = [P, P, P, I32, I64, ctypes.c_double, P, P, P]
    L.wab_bush_thresholds.argtypes = [ctypes.c_double, I32, P]
    L.wab_rollout_features.argtypes = [P, P, I32, P, P, P, P, ctypes.c_double, P, P, P]
    L.wab_batch.argtypes = [P]
    L.wab_batch.restype = I64
    L.wab_step_kernel.argtypes = [P]
    L.wab_step_kernel.restype = ctypes.c_char_p
    L.wab_set_obs_placement.argtypes = [P, I32]
    L.wab_snapshot_bytes.argtypes = [P]
    L.wab_snapshot_hash.argtypes = [P]
    L.wab_snapshot_hash.restype = U64
    L.wab_snapshot_save.argtypes = [P, I64, I64, P, P, P]
    L.wab_snapshot_restore.argtypes = [P, P, P, P, P]
    L.wab_policy_create.argtypes = [P, ctypes.c_int, ctypes.POINTER(P)]
    L.wab_policy_load.argtypes = [P, P, P]
    L.wab_policy_act.argtypes = [P, P, P, P, P, P, P]
    L.wab_policy_destroy.argtypes = [P]
    L.wab_policy_set_action_rule.argtypes = [P, P]
    L.wab_policy_get_action_rule.argtypes = [P, P]
    L.wab_rollout_policy_fused.argtypes = [P, P]
    L.wab_rollout_policy.argtypes = [P, P, P, I32, P, P, P, P, P, P, P, P, ctypes.c_double, P, P, P]
    L.wab_debug_returns_plan.argtypes = [P, P, P, P, I64, P]
    L.wab_debug_policy_plan.argtypes = [P, P]
    L.wab_episode_stats_workspace.argtypes = [I32, I64]
    L.wab_episode_stats_workspace.restype = I64
    L.wab_episode_stats_update.argtypes = [P, P, P, I32, I64, P, P, P, P, P, P, I64, P, P, P]
    L.wab_normalize_episode_returns.argtypes = [P, P, I32, I64, ctypes.c_double, P, P]
    L.wab_gae.argtypes = [P, P, P, P, P, I32, I64, ctypes.c_double, ctypes.c_double, P, P, P]
    L.wab_whiten_workspace.argtypes = [I64]
    L.wab_whiten_workspace.restype = I64
    L.wab_whiten.argtypes = [P, I64, ctypes.c_double, P, P, P]
    L.wab_debug_gae_plan.argtypes = [P, P, P, P, P, P, I64, P]
    L.wab_policy_grad_workspace.argtypes = [P, I64, I32]
    L.wab_policy_grad_workspace.restype = ctypes.c_size_t
    L.wab_policy_grad.argtypes = [P, P, P, P, P, I64, P, P, P, P, P, P, P, ctypes.c_size_t, P]
    L.wab_policy_grad_bad_actions.argtypes = [P, P, P, P]
    L.wab_policy_grad_ppo.argtypes = [P, P, P, P, P, P, P, I64, P, P, P, P, P, P, P, P, P, P, ctypes.c_size_t, P]
    L.wab_policy_evaluate.argtypes = [P, P, P, I64, P, P, P, P, ctypes.c_size_t, P]
    # the contiguous calls' arguments, then rows (int32 [N]) and M
    L.wab_policy_grad_gather.argtypes = L.wab_policy_grad.argtypes + [P, I64]
    L.wab_policy_grad_ppo_gather.argtypes = L.wab_policy_grad_ppo.argtypes + [P, I64]
    L.wab_policy_evaluate_gather.argtypes = L.wab_policy_evaluate.argtypes + [P, I64]
    L.wab_policy_grad_bad_rows.argtypes = [P, P, P, P]
    # the _gather calls' arguments, feature_bits (uint32 [M][P]) in place of features; rows may be NULL
    L.wab_policy_grad_packed.argtypes = L.wab_policy_grad_gather.argtypes
    L.wab_policy_grad_ppo_packed.argtypes = L.wab_policy_grad_ppo_gather.argtypes
    L.wab_policy_evaluate_packed.argtypes = L.wab_policy_evaluate_gather.argtypes
    L.wab_feature_bits_pitch.argtypes = [I32]
    L.wab_features_pack.argtypes = [P, I64, I32, P, P, P]
    L.wab_features_unpack.argtypes = [P, I64, I32, P, P]
    L.wab_rollout_policy_packed.argtypes = L.wab_rollout_policy.argtypes
    L.wab_debug_policy_grad_plan.argtypes = [P, I32, P]
    L.wab_policy_adam_workspace.argtypes = [P]
    L.wab_policy_adam_workspace.restype = ctypes.c_size_t
    L.wab_policy_adam_step.argtypes = [P, P, P, P, P, P, P, P, ctypes.c_size_t, P]
    L.wab2_last_error.restype = ctypes.c_char_p
    L.wab2_record_size.argtypes = [P]
    L.wab2_create.argtypes = [P, I64, U64, I64, ctypes.c_int, ctypes.POINTER(P)]
    L.wab2_destroy.argtypes = [P]
    L.wab2_batch.argtypes = [P]
    L.wab2_batch.restype = I64
    L.wab2_reset.argtypes = [P, P, P]
    L.wab2_create_at.argtypes = [P, I64, U64, I64, ctypes.c_int, P, ctypes.POINTER(P)]
    L.wab2_reset_at.argtypes = [P, P, P, P]
    L.wab2_step.argtypes = [P, P, P, P, P, P, P]
    L.wab2_rollout.argtypes = [P, P, I32, P, P, P, P, P]
    L.wab2_get_state.argtypes = [P] * 9
    L.wab2_get_counters.argtypes = [P, P, P]
    L.wab2_get_obs.argtypes = [P, I32, P, P]
    L.wab2_take_action.argtypes = [P, I32, P, P, P, P, P]
    for name in EXPORTED:  # (all there; c_int, ctypes' default, stands where no restype is given above)
        getattr(L, name)
    if L.wab_abi_version() != ABI_VERSION:
        raise WabError("libwab_hip.so ABI %d != %d" % (L.wab_abi_version(), ABI_VERSION))
    if L.wab2_abi_version() != ABI2_VERSION:
        raise WabError("libwab_hip.so torus ABI %d != %d" % (L.wab2_abi_version(), ABI2_VERSION))
    _lib = L
    return L


class Wab2Counters(ctypes.Structure):
    _fields_ = [("turns", ctypes.c_uint64), ("resets", ctypes.c_uint64)]


def check2(rc, what="wab2 call"):
    """check() for the torus entry points (their own wab2_last_error)."""
    if rc != 0:
        msg = load().wab2_last_error().decode(errors="replace")
        if rc == -1:
            raise ValueError("%s: %s" % (what, msg))
        raise WabError("%s failed (%d): %s" % (what, rc, msg))


def check(rc, what="wab call"):
    if rc != 0:
        msg = load().wab_last_error().decode(errors="replace")
        if rc == -1:
            raise ValueError("%s: %s" % (what, msg))
        raise WabError("%s failed (%d): %s" % (what, rc, msg))
