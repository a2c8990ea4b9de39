"""MI355X-native batched step() engine for the MARL-SortingEnv environments.

Hot path only: the per-env state transition of Env_1_Sorting /
Env_2_Pressing / Env_3_Monolith as hand-written HIP kernels behind a C ABI (include/mse.h),
with the reference's Gymnasium reset()/step()/action_masks() surface on the host side.
"""
from ._lib import (MSE_ENV_MONO, MSE_ENV_PRESS, MSE_ENV_SORT, MSE_SNAP_INTS, MSE_STEP_CHECK_OVERFLOW,
                   MSE_STEP_UNMASKED, MseError, library_path, load_library)
from .build import build_library
from .config import KIND_BY_NAME, NUM_ACTIONS, OBS_DIM, SortingEnvConfig

__all__ = [
    "BatchedSortingEnv", "Env_1_Sorting", "Env_2_Pressing", "Env_3_Monolith", "SortingVecEnv",
    "ShardedSortingEnv", "GradientExchange", "shard_minibatch_plan", "MlpPolicy", "PolicyRolloutCollector", "FusedPolicyRollout", "ModelRolloutCollector", "FusedModularRollout", "ModularRolloutCollector", "ModularTrainer", "PPOLearner", "PPO_BC_STAT_NAMES", "DemonstrationCollector", "FusedDemonstrationRollout", "expert_threshold", "ImitationLearner", "compute_gae", "resolve_schedule", "EpisodeStats", "evaluate_policy", "evaluate_rollout", "PlantStats", "evaluate_plant", "lookahead_reference", "LookaheadCollector", "evaluate_lookahead", "EnvTrace", "save_checkpoint", "load_checkpoint", "SortingEnvConfig", "MseError", "build_library", "load_library", "library_path",
    "KIND_BY_NAME", "OBS_DIM", "NUM_ACTIONS", "MSE_ENV_SORT", "MSE_ENV_PRESS", "MSE_ENV_MONO",
    "MSE_STEP_UNMASKED", "MSE_STEP_CHECK_OVERFLOW", "MSE_SNAP_INTS",
]


def __getattr__(name):  # torch-dependent front-ends are imported on first use
    if name == "BatchedSortingEnv":
        from .batched import BatchedSortingEnv
        return BatchedSortingEnv
    if name in ("Env_1_Sorting", "Env_2_Pressing", "Env_3_Monolith"):
        from . import envs
        return getattr(envs, name)
    if name == "SortingVecEnv":
        from .vec_env import SortingVecEnv
        return SortingVecEnv
    if name in ("PolicyRolloutCollector", "FusedPolicyRollout", "ModelRolloutCollector", "FusedModularRollout",
                "ModularRolloutCollector"):
        from . import collector
        return getattr(collector, name)
    if name == "ModularTrainer":
        from .modular import ModularTrainer
        return ModularTrainer
    if name in ("PPOLearner", "PPO_BC_STAT_NAMES", "compute_gae", "resolve_schedule"):
        from . import learner
        return getattr(learner, name)
    if name in ("DemonstrationCollector", "FusedDemonstrationRollout", "expert_threshold", "ImitationLearner"):
        from . import imitation
        return getattr(imitation, name)
    if name in ("EpisodeStats", "evaluate_policy", "evaluate_rollout"):
        from . import episodes
        return getattr(episodes, name)
    if name in ("PlantStats", "evaluate_plant"):
        from . import plant
        return getattr(plant, name)
    if name in ("lookahead_reference", "LookaheadCollector", "evaluate_lookahead"):
        from . import lookahead
        return getattr(lookahead, name)
    if name == "EnvTrace":
        from .trace import EnvTrace
        return EnvTrace
    if name in ("save_checkpoint", "load_checkpoint"):
        from . import checkpoint
        return getattr(checkpoint, name)
    if name == "MlpPolicy":
        from .policy import MlpPolicy
        return MlpPolicy
    if name in ("ShardedSortingEnv", "GradientExchange", "shard_minibatch_plan"):
        from . import sharding
        return getattr(sharding, name)
    raise AttributeError(name)
