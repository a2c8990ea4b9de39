"""CPU checks of the lookahead with a network (no device needed): the refusals of `mse_lookahead_net` that need no handle,
through the library, and what `BatchedSortingEnv.lookahead`, `LookaheadCollector`, `evaluate_lookahead` and
`lookahead_reference` refuse in Python before anything is stepped: two different policies for base and leaf, a policy of
the wrong shape or device, an unknown keyword, a base_policy string other than the two known ones."""
import ctypes as C
import types

import numpy as np
import pytest

INVALID = -1


@pytest.fixture(scope="module")
def lib():
    import marl_sortingenv_amd as M

    return M.load_library()


def _net_call(lib, env, policy, horizon=4, gamma=1.0, base=2, det=1, base_seed=2024, leaf=1, streams=1, seed=0, m=1, sort_mode=None,
              flags=0, q=None, action=None, value=None, ws=None):
    return lib.mse_lookahead_net(env, policy, horizon, gamma, base, det, base_seed, leaf, streams, seed, m, sort_mode, flags, q, action,
                                 value, ws, None)


def test_refusals_that_need_no_handle(lib):
    q = np.full(8, 7.0)
    ws = np.full(8, 7.0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    # a NULL env is the first refusal, whatever else is right or wrong
    assert _net_call(lib, None, None, q=p(q), ws=p(ws)) == INVALID
    assert b"mse_lookahead_net" in lib.mse_last_error() and b"NULL" in lib.mse_last_error()
    assert _net_call(lib, None, None, horizon=0, gamma=2.0, base=5, leaf=7, streams=5, m=0, flags=255) == INVALID
    assert b"mse_lookahead_net" in lib.mse_last_error() and b"NULL" in lib.mse_last_error()
    assert (q == 7.0).all() and (ws == 7.0).all()


def test_the_symbol_is_bound_with_the_headers_signature(lib):
    from marl_sortingenv_amd import _lib

    assert "mse_lookahead_net" in _lib.EXPORTS
    # env, policy, horizon, gamma, base_policy, base_deterministic, base_seed, leaf_value, streams, lookahead_seed, n_samples,
    # sort_mode_dev, flags, q_out, action_out, value_out, workspace, stream
    assert len(lib.mse_lookahead_net.argtypes) == 18
    assert lib.mse_lookahead_net.argtypes[3] is C.c_double


def _fake_env(**over):
    import torch

    base = dict(auto_reset=True, obs_dim=29, num_actions=22, num_envs=4, kind="mono", device=torch.device("cuda", 0))
    return types.SimpleNamespace(**dict(base, **over))


def _fake_policy(obs_dim=29, n_actions=22, device=("cuda", 0)):
    import torch

    return types.SimpleNamespace(obs_dim=obs_dim, n_actions=n_actions, device=torch.device(*device))


def test_lookahead_refuses_in_python_before_the_library():
    from marl_sortingenv_amd.batched import BatchedSortingEnv

    env = _fake_env()  # no handle: a refusal that came later than these would raise AttributeError instead
    p, other = _fake_policy(), _fake_policy()
    with pytest.raises(ValueError, match="same MlpPolicy"):
        BatchedSortingEnv.lookahead(env, 4, base_policy=p, leaf_value=other)
    for wrong in (_fake_policy(obs_dim=16, n_actions=11), _fake_policy(n_actions=11), _fake_policy(obs_dim=13)):
        with pytest.raises(ValueError, match="29 -> 22"):
            BatchedSortingEnv.lookahead(env, 4, base_policy=wrong)
        with pytest.raises(ValueError, match="29 -> 22"):
            BatchedSortingEnv.lookahead(env, 4, leaf_value=wrong)
        with pytest.raises(ValueError, match="29 -> 22"):
            BatchedSortingEnv.lookahead(env, 4, base_policy=wrong, leaf_value=wrong)
    for elsewhere in (_fake_policy(device=("cuda", 1)), _fake_policy(device=("cpu",))):
        with pytest.raises(ValueError, match="policy on cuda:0"):
            BatchedSortingEnv.lookahead(env, 4, base_policy="rule_based", leaf_value=elsewhere)
    # a string other than the two known ones: the ValueError it always was; something that is neither a string nor a policy
    with pytest.raises(ValueError, match="base_policy must be 'rule_based' or 'random', not 'greedy'"):
        BatchedSortingEnv.lookahead(env, 4, base_policy="greedy", leaf_value=p)
    with pytest.raises(ValueError, match="base_policy must be 'rule_based' or 'random', not 'network'"):
        BatchedSortingEnv.lookahead(env, 4, base_policy="network")
    for junk in (None, 2, object()):
        with pytest.raises(ValueError, match="base_policy"):
            BatchedSortingEnv.lookahead(env, 4, base_policy=junk)
    with pytest.raises(ValueError, match="leaf_value"):
        BatchedSortingEnv.lookahead(env, 4, leaf_value="critic")
    with pytest.raises(TypeError):
        BatchedSortingEnv.lookahead(env, 4, leaf=p)
    # the older refusals still come, with a network in the call
    with pytest.raises(ValueError, match="streams"):
        BatchedSortingEnv.lookahead(env, 4, base_policy=p, leaf_value=p, streams="new")
    with pytest.raises(ValueError, match="horizon"):
        BatchedSortingEnv.lookahead(env, 0, base_policy=p)
    with pytest.raises(ValueError, match="n_samples"):
        BatchedSortingEnv.lookahead(env, 4, leaf_value=p, n_samples=0)


def test_keyword_list_and_argument_check():
    from marl_sortingenv_amd.lookahead import LOOKAHEAD_KW, check_lookahead_args

    assert LOOKAHEAD_KW[:8] == ("gamma", "base_policy", "streams", "seed", "base_seed", "n_samples", "sort_mode", "check_overflow")
    assert set(LOOKAHEAD_KW[8:]) == {"leaf_value", "base_deterministic"}
    p, other = _fake_policy(), _fake_policy()
    check_lookahead_args(4, dict(base_policy=p, leaf_value=p, base_deterministic=False))
    check_lookahead_args(1, dict(base_policy="random", leaf_value=p))
    check_lookahead_args(1, dict(base_policy=p))
    with pytest.raises(ValueError, match="same MlpPolicy"):
        check_lookahead_args(4, dict(base_policy=p, leaf_value=other))
    with pytest.raises(ValueError, match="base_policy must be 'rule_based' or 'random', not 'greedy'"):
        check_lookahead_args(4, dict(base_policy="greedy"))
    with pytest.raises(TypeError, match="unknown lookahead argument"):
        check_lookahead_args(4, dict(leaf=p))


def test_collector_evaluation_and_twin_refusals():
    from marl_sortingenv_amd.lookahead import LookaheadCollector, evaluate_lookahead, lookahead_reference

    env = _fake_env()
    p, other = _fake_policy(), _fake_policy()
    with pytest.raises(ValueError, match="same MlpPolicy"):
        LookaheadCollector(env, 8, 4, actor=p, base_policy=p, leaf_value=other)
    with pytest.raises(ValueError, match="base_policy"):
        LookaheadCollector(env, 8, 4, base_policy="greedy", leaf_value=p)
    with pytest.raises(TypeError, match="unknown lookahead argument"):
        LookaheadCollector(env, 8, 4, base_policy=p, leaf_policy=p)
    with pytest.raises(TypeError, match="unknown lookahead argument"):
        LookaheadCollector(env, 8, 4, gamma=0.9, seed=1, leaf_value=p, base_determinist=True)
    with pytest.raises(ValueError, match="same MlpPolicy"):
        evaluate_lookahead(env, 10, 4, base_policy=p, leaf_value=other)
    with pytest.raises(TypeError, match="unknown lookahead argument"):
        evaluate_lookahead(env, 10, 4, leaf=p)
    with pytest.raises(ValueError, match="same MlpPolicy"):
        lookahead_reference(env, 4, base_policy=p, leaf_value=other)
    with pytest.raises(ValueError, match="base_policy"):
        lookahead_reference(env, 4, base_policy="greedy", leaf_value=p)
