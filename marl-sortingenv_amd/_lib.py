"""ctypes binding of libmse_hip.so (include/mse.h).  No CPU fallback: a missing library is an error."""
from __future__ import annotations

import ctypes as C
import os

from .build import LIB_PATH

MSE_ENV_SORT, MSE_ENV_PRESS, MSE_ENV_MONO = 1, 2, 3
MSE_STEP_UNMASKED, MSE_STEP_CHECK_OVERFLOW, MSE_ROLLOUT_RULE_BASED, MSE_STEP_SANITIZE_LATE = 1, 2, 4, 8
MSE_MODEL_NO_SORT_DRAW, MSE_MODEL_NO_PRESS_DRAW = 16, 32
MSE_MODEL_PRESS_AGENT_MASKED = 64
MSE_MODULAR_SORT_DETERMINISTIC, MSE_MODULAR_PRESS_DETERMINISTIC = 128, 256
MSE_DEMO_ACTOR_DETERMINISTIC = 512
MSE_PREVIEW_DETERMINISTIC = 1024
MSE_SNAP_INTS = 71
MSE_SNAP_RNG_WORDS = 30  # rng, rng_noise, rng_pressing, rng_sorting, input generator x {state_hi, state_lo, inc_hi, inc_lo, has_uint32, uinteger}
MSE_TRACE_COLS = 40
MSE_PLANT_COLS, MSE_PLANT_RUN_COLS = 32, 36
MSE_LOOKAHEAD_MAX_HORIZON, MSE_LOOKAHEAD_MAX_SAMPLES = 65535, 256

EXPORTS = [
    "mse_version", "mse_last_error", "mse_status_string", "mse_config_default", "mse_create",
    "mse_create_indexed", "mse_destroy", "mse_num_envs", "mse_obs_dim", "mse_num_actions", "mse_reset",
    "mse_step", "mse_action_masks", "mse_rollout", "mse_sample_actions", "mse_rule_actions", "mse_get_state", "mse_set_state",
    "mse_error_count", "mse_algorithmic_bytes_per_step", "mse_tie_window",
    "mse_sort_agent_obs", "mse_policy_num_weights", "mse_policy_create", "mse_policy_destroy", "mse_policy_forward",
    "mse_get_policy_step", "mse_set_policy_step", "mse_model_actions", "mse_trace_begin", "mse_trace_end", "mse_press_agent_obs", "mse_rollout_policy", "mse_policy_set_precision", "mse_policy_precision",
    "mse_rollout_model", "mse_rollout_modular", "mse_rollout_modular_check",
    "mse_policy_set_weights", "mse_gae", "mse_ppo_workspace_bytes", "mse_ppo_loss_grad", "mse_ppo_adam_step",
    "mse_ppo_shuffle", "mse_ppo_shuffle_host",
    "mse_policy_set_weights_device", "mse_policy_sync", "mse_policy_image_floats", "mse_policy_pack_host",
    "mse_policy_read_image", "mse_policy_get_weights", "mse_ppo_loss_grad_gated", "mse_ppo_adam_step_gated",
    "mse_episode_workspace_bytes", "mse_episode_scan", "mse_episode_scan_host", "mse_episode_summary", "mse_episode_summary_host",
    "mse_ppo_loss_grad_matrix",
    "mse_ppo_loss_grad_vclip", "mse_explained_variance_workspace_bytes", "mse_explained_variance", "mse_explained_variance_host",
    "mse_bc_loss_grad", "mse_ppo_bc_workspace_bytes", "mse_ppo_bc_loss_grad",
    "mse_rollout_demo", "mse_rollout_demo_check", "mse_demo_who_steps_host",
    "mse_rollout_policy_labelled", "mse_rollout_policy_labelled_check",
    "mse_rollout_modular_labelled", "mse_rollout_modular_labelled_check",
    "mse_mono_agent_obs", "mse_rollout_policy_preview", "mse_rollout_policy_preview_check",
    "mse_trace_begin_all", "mse_plant_workspace_bytes", "mse_plant_scan", "mse_plant_scan_host", "mse_plant_params",
    "mse_ppo_shard_partial_len", "mse_ppo_shard_moments", "mse_ppo_shard_loss_grad", "mse_ppo_shard_finish",
    "mse_lookahead_workspace_bytes", "mse_lookahead_stream_seed", "mse_lookahead",
    "mse_lookahead_net",
]

_other_libs: dict = {}


class MseError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"libmse_hip status {status}: {message}")
        self.status = status


class MseConfigStruct(C.Structure):
    """struct mse_config (include/mse.h)"""
    _fields_ = [
        ("struct_size", C.c_uint32), ("env_kind", C.c_int32), ("max_steps", C.c_int32),
        ("auto_reset", C.c_int32), ("track_bales", C.c_int32), ("literal_choice", C.c_int32),
        ("input_batch_size", C.c_int32), ("steps_per_pattern", C.c_int32),
        ("baseline_accuracy", C.c_double * 4), ("boost", C.c_double), ("noise", C.c_double),
        ("stage_capacity", C.c_int32),
        ("press_time", C.c_int32 * 2), ("container_capacity", C.c_int32), ("bale_standard_size", C.c_int32),
        ("bale_remainder_threshold", C.c_double), ("quality_threshold", C.c_double * 4),
        ("quality_threshold_r2", C.c_double * 4),
        ("purity_threshold_theta", C.c_double), ("tanh_temperature", C.c_double),
        ("overflow_penalty_catastrophic", C.c_double), ("overflow_penalty_severe", C.c_double),
        ("overflow_penalty_mild", C.c_double), ("bale_efficiency_factor", C.c_double),
        ("max_state_reward", C.c_double), ("overflow_termination_penalty", C.c_double),
        ("pattern_ratio", (C.c_double * 4) * 2),
        ("rollout_pipeline", C.c_int32), ("reserved0", C.c_int32),
    ]


class MsePpoParams(C.Structure):
    """struct mse_ppo_params (include/mse.h)"""
    _fields_ = [("struct_size", C.c_uint32), ("clip_range", C.c_float), ("ent_coef", C.c_float), ("vf_coef", C.c_float),
                ("normalize_advantage", C.c_int32)]


# the pointer members of struct mse_modular_buffers, in the header's order (= the keys of the collectors' buffer dicts)
MODULAR_BUFFER_NAMES = ("sort_obs", "press_obs", "press_masks", "episode_starts", "sort_actions", "press_actions",
                        "sort_log_probs", "press_log_probs", "sort_values", "press_values", "rewards", "rewards_sort",
                        "rewards_press", "sort_last_values", "press_last_values", "last_dones")


class MseModularBuffers(C.Structure):
    """struct mse_modular_buffers (include/mse.h)"""
    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_uint32)] + [(name, C.c_void_p) for name in MODULAR_BUFFER_NAMES]


# the pointer members of struct mse_demo_buffers, in the header's order
DEMO_BUFFER_NAMES = ("observations", "action_masks", "episode_starts", "labels", "stepped_actions", "expert_stepped",
                     "rewards", "last_dones")


class MseDemoBuffers(C.Structure):
    """struct mse_demo_buffers (include/mse.h)"""
    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_uint32)] + [(name, C.c_void_p) for name in DEMO_BUFFER_NAMES]


# the pointer members of struct mse_modular_label_buffers, in the header's order (= the keys a labelled modular collector adds)
MODULAR_LABEL_BUFFER_NAMES = ("sort_expert_actions", "press_expert_actions", "stepped_actions", "expert_stepped")


class MseModularLabelBuffers(C.Structure):
    """struct mse_modular_label_buffers (include/mse.h)"""
    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_uint32)] + \
               [(name, C.c_void_p) for name in MODULAR_LABEL_BUFFER_NAMES]


# the pointer members of struct mse_preview_buffers, in the header's order (= the keys of the preview collectors' buffer dicts)
PREVIEW_BUFFER_NAMES = ("observations", "action_masks", "episode_starts", "actions", "log_probs", "values", "rewards",
                        "expert_actions", "stepped_actions", "expert_stepped", "last_values", "last_dones")


class MsePreviewBuffers(C.Structure):
    """struct mse_preview_buffers (include/mse.h)"""
    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_uint32)] + [(name, C.c_void_p) for name in PREVIEW_BUFFER_NAMES]


_lib = None


def library_path() -> str:
    return LIB_PATH


def load_library(path: str | None = None) -> C.CDLL:
    """Loads the in-tree libmse_hip.so; raises if it has not been built (python -m ... build).
    `path` names another build of the same source (tests load libmse_hip_widetie.so beside the product)."""
    global _lib
    if path is None and _lib is not None:
        return _lib
    if path is not None and path in _other_libs:
        return _other_libs[path]
    lib_path = LIB_PATH if path is None else path
    if not os.path.exists(lib_path):
        raise ImportError(
            f"{lib_path} is missing: build it with `python __graft_entry__.py` or "
            "`python marl-sortingenv_amd/build.py`. There is no CPU fallback for the step path.")
    # PyTorch-ROCm bundles its own HIP runtime (same SONAME as ROCm's). Import it first so that
    # libmse_hip.so binds to the runtime torch uses: streams and device pointers are shared objects.
    import torch  # noqa: F401

    L = C.CDLL(lib_path)
    vp, i32, i64, u32, u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64
    L.mse_version.restype = C.c_int
    L.mse_last_error.restype = C.c_char_p
    L.mse_status_string.argtypes = [C.c_int]
    L.mse_status_string.restype = C.c_char_p
    L.mse_config_default.argtypes = [C.POINTER(MseConfigStruct)]
    L.mse_create.argtypes = [C.POINTER(vp), C.POINTER(MseConfigStruct), i64, C.c_int]
    L.mse_create_indexed.argtypes = [C.POINTER(vp), C.POINTER(MseConfigStruct), i64, C.c_int, i64]
    L.mse_destroy.argtypes = [vp]
    L.mse_num_envs.argtypes = [vp]
    L.mse_num_envs.restype = i64
    L.mse_obs_dim.argtypes = [vp]
    L.mse_num_actions.argtypes = [vp]
    L.mse_reset.argtypes = [vp, vp, vp, vp, vp, vp]
    L.mse_step.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp]
    L.mse_action_masks.argtypes = [vp, vp, vp]
    L.mse_sort_agent_obs.argtypes = [vp, vp, vp]
    L.mse_press_agent_obs.argtypes = [vp, vp, vp]
    L.mse_mono_agent_obs.argtypes = [vp, vp, vp]
    L.mse_rollout.argtypes = [vp, i32, u64, vp, u32, vp, vp, vp, vp, vp, vp]
    L.mse_sample_actions.argtypes = [vp, u64, vp, vp]
    L.mse_rule_actions.argtypes = [vp, vp, vp]
    L.mse_get_state.argtypes = [vp, vp, vp, vp, vp]
    L.mse_set_state.argtypes = [vp, vp, vp, vp, vp]
    L.mse_error_count.argtypes = [vp, C.POINTER(u64)]
    L.mse_algorithmic_bytes_per_step.argtypes = [vp]
    L.mse_get_policy_step.argtypes = [vp, C.POINTER(u64)]
    L.mse_set_policy_step.argtypes = [vp, u64]
    L.mse_model_actions.argtypes = [vp, u32, vp, vp]
    L.mse_trace_begin.argtypes = [vp, i64, vp, i64]
    L.mse_trace_end.argtypes = [vp, C.POINTER(i64)]
    L.mse_trace_begin_all.argtypes = [vp, vp, i64]
    for name in EXPORTS:
        getattr(L, name)  # AttributeError if the library does not export what include/mse.h declares
    L.mse_tie_window.restype = u32
    L.mse_policy_num_weights.argtypes = [C.c_int, C.c_int]
    L.mse_policy_num_weights.restype = i64
    L.mse_policy_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int]
    L.mse_policy_destroy.argtypes = [vp]
    L.mse_policy_set_precision.argtypes = [vp, C.c_int]
    L.mse_policy_precision.argtypes = [vp]
    L.mse_policy_forward.argtypes = [vp, i64, i64, vp, vp, u64, u64, C.c_int, vp, vp, vp, vp, vp]
    L.mse_rollout_policy.argtypes = [vp, vp, vp, i32, u64, C.c_int, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.mse_rollout_model.argtypes = [vp, vp, vp, i32, u32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.mse_rollout_modular.argtypes = [vp, vp, vp, i32, u64, u64, u32, C.POINTER(MseModularBuffers), vp]
    L.mse_rollout_modular_check.argtypes = [vp, vp, vp, i32, u64, u64, u32]
    L.mse_rollout_modular_labelled.argtypes = [vp, vp, vp, i32, u64, u64, u64, u32, u32, C.POINTER(MseModularBuffers),
                                               C.POINTER(MseModularLabelBuffers), vp]
    L.mse_rollout_modular_labelled_check.argtypes = [vp, vp, vp, i32, u64, u64, u64, u32, u32]
    L.mse_rollout_demo.argtypes = [vp, vp, i32, u64, u64, u32, u32, C.POINTER(MseDemoBuffers), vp]
    L.mse_rollout_demo_check.argtypes = [vp, vp, i32, u64, u64, u32, u32]
    L.mse_rollout_policy_labelled.argtypes = [vp, vp, i32, u64, C.c_int, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.mse_rollout_policy_labelled_check.argtypes = [vp, vp, i32, u64, C.c_int, vp, u32]
    L.mse_rollout_policy_preview.argtypes = [vp, vp, i32, u64, u64, u32, u32, C.POINTER(MsePreviewBuffers), vp]
    L.mse_rollout_policy_preview_check.argtypes = [vp, vp, i32, u64, u64, u32, u32]
    L.mse_demo_who_steps_host.argtypes = [i64, i64, u64, u64, u32, vp]
    L.mse_policy_set_weights.argtypes = [vp, C.POINTER(C.c_float)]
    L.mse_policy_set_weights_device.argtypes = [vp, vp, vp]
    L.mse_policy_sync.argtypes = [vp]
    L.mse_policy_image_floats.argtypes = []
    L.mse_policy_image_floats.restype = i64
    L.mse_policy_pack_host.argtypes = [C.c_int, C.c_int, vp, vp, vp]
    L.mse_policy_read_image.argtypes = [vp, vp]
    L.mse_policy_get_weights.argtypes = [vp, vp]
    L.mse_gae.argtypes = [i32, i64, vp, vp, vp, vp, vp, C.c_double, C.c_double, vp, vp, vp]
    L.mse_ppo_workspace_bytes.argtypes = [C.c_int, C.c_int]
    L.mse_ppo_workspace_bytes.restype = i64
    L.mse_ppo_loss_grad.argtypes = [C.c_int, C.c_int, vp, i64, vp, i64, vp, vp, vp, vp, vp, vp, C.POINTER(MsePpoParams), vp, vp, vp, vp]
    L.mse_ppo_adam_step.argtypes = [i64, vp, vp, vp, vp, i64, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, vp, vp]
    L.mse_ppo_loss_grad_gated.argtypes = L.mse_ppo_loss_grad.argtypes + [C.c_double, vp]
    L.mse_ppo_adam_step_gated.argtypes = L.mse_ppo_adam_step.argtypes + [vp]
    L.mse_ppo_loss_grad_matrix.argtypes = L.mse_ppo_loss_grad_gated.argtypes
    L.mse_ppo_loss_grad_vclip.argtypes = L.mse_ppo_loss_grad_gated.argtypes + [C.c_int, vp, C.c_double]
    L.mse_ppo_shard_partial_len.argtypes = [C.c_int, C.c_int]
    L.mse_ppo_shard_partial_len.restype = i64
    L.mse_ppo_shard_moments.argtypes = [i64, vp, i64, vp, vp, vp, vp, vp]
    L.mse_ppo_shard_loss_grad.argtypes = L.mse_ppo_loss_grad.argtypes[:13] + [i64, vp, vp, vp, vp, vp, C.c_int, vp, C.c_double]
    L.mse_ppo_shard_finish.argtypes = [C.c_int, C.c_int, i64, vp, vp, C.POINTER(MsePpoParams), vp, vp, vp, C.c_double, vp]
    L.mse_ppo_bc_workspace_bytes.argtypes = [C.c_int, C.c_int]
    L.mse_ppo_bc_workspace_bytes.restype = i64
    L.mse_ppo_bc_loss_grad.argtypes = L.mse_ppo_loss_grad_vclip.argtypes + [vp, C.c_double]
    L.mse_bc_loss_grad.argtypes = [C.c_int, C.c_int, vp, i64, vp, i64, vp, vp, vp, vp, C.POINTER(MsePpoParams), vp, vp, vp, vp, C.c_int]
    L.mse_explained_variance_workspace_bytes.argtypes = []
    L.mse_explained_variance_workspace_bytes.restype = i64
    L.mse_explained_variance.argtypes = [i64, vp, vp, vp, vp, vp]
    L.mse_explained_variance_host.argtypes = [i64, vp, vp, vp]
    L.mse_ppo_shuffle.argtypes = [i64, u64, u64, i64, i64, vp, vp]
    L.mse_ppo_shuffle_host.argtypes = [i64, u64, u64, i64, i64, vp]
    L.mse_episode_workspace_bytes.argtypes = []
    L.mse_episode_workspace_bytes.restype = i64
    L.mse_episode_scan.argtypes = [i32, i64, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp]
    L.mse_episode_scan_host.argtypes = [i32, i64, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp]
    L.mse_episode_summary.argtypes = [i64, i32, vp, vp, vp, vp, vp]
    L.mse_episode_summary_host.argtypes = [i64, i32, vp, vp, vp, vp]
    L.mse_plant_workspace_bytes.argtypes = []
    L.mse_plant_workspace_bytes.restype = i64
    L.mse_plant_scan.argtypes = [i32, i64, vp, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp]
    L.mse_plant_scan_host.argtypes = [i32, i64, vp, i32, i32, vp, vp, vp, i32, vp, vp]
    L.mse_plant_params.argtypes = [vp, C.POINTER(i32 * 2)]
    L.mse_lookahead_workspace_bytes.argtypes = [vp, i32]
    L.mse_lookahead_workspace_bytes.restype = i64
    L.mse_lookahead_stream_seed.argtypes = [u64, u64, u32]
    L.mse_lookahead_stream_seed.restype = u64
    L.mse_lookahead.argtypes = [vp, i32, C.c_double, i32, u64, i32, u64, i32, vp, u32, vp, vp, vp, vp, vp]
    L.mse_lookahead_net.argtypes = [vp, vp, i32, C.c_double, i32, i32, u64, i32, i32, u64, i32, vp, u32, vp, vp, vp, vp, vp]
    if path is None:
        _lib = L
    else:
        _other_libs[path] = L
    return L


def check(status: int):
    if status != 0:
        raise MseError(status, load_library().mse_last_error().decode(errors="replace"))
