"""CPU: the host-only logic of the modular collection - the views a learner is handed (names, aliasing, which reward),
the argument rules both collectors and the trainer check before any handle is asked, and the ctypes mirror of
struct mse_modular_buffers against include/mse.h.  No device, no library call."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import pytest
import torch

from marl_sortingenv_amd import _lib
from marl_sortingenv_amd.collector import _check_modular, _modular_buffers, modular_view
from marl_sortingenv_amd.modular import ModularTrainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIEW_KEYS = {"observations", "action_masks", "actions", "log_probs", "values", "rewards", "episode_starts", "last_values",
             "last_dones"}


def test_views_alias_the_buffers_under_the_learner_names():
    b = _modular_buffers(5, 3, "cpu")
    assert set(b) == set(_lib.MODULAR_BUFFER_NAMES)
    for who, D, A in (("sort", 13, 2), ("press", 16, 11)):
        for reward in ("own", "team"):
            v = modular_view(b, who, reward)
            assert set(v) == VIEW_KEYS
            assert v["observations"] is b[f"{who}_obs"] and tuple(v["observations"].shape) == (3, 5, D)
            assert v["actions"] is b[f"{who}_actions"] and v["log_probs"] is b[f"{who}_log_probs"]
            assert v["values"] is b[f"{who}_values"] and v["last_values"] is b[f"{who}_last_values"]
            assert v["episode_starts"] is b["episode_starts"] and v["last_dones"] is b["last_dones"]
            assert v["rewards"] is (b["rewards"] if reward == "team" else b[f"rewards_{who}"])
    assert modular_view(b, "sort")["action_masks"] is None
    assert modular_view(b, "press")["action_masks"] is b["press_masks"]
    assert modular_view(b, "press", press_masked=False)["action_masks"] is None
    # a write through the view lands in the buffer: nothing was copied
    modular_view(b, "press")["rewards"].fill_(7.0)
    assert bool((b["rewards_press"] == 7.0).all())


def test_view_argument_checks():
    b = _modular_buffers(2, 2, "cpu")
    with pytest.raises(ValueError, match="who"):
        modular_view(b, "presser")
    with pytest.raises(ValueError, match="reward"):
        modular_view(b, "sort", reward="shared")
    twin = _modular_buffers(2, 2, "cpu", parts=False)  # the multi-launch twin fills no reward parts
    assert "rewards_sort" not in twin and "rewards_press" not in twin
    with pytest.raises(KeyError):
        modular_view(twin, "sort", "own")
    assert modular_view(twin, "sort", "team")["rewards"] is twin["rewards"]


def _fake(kind="mono", auto_reset=True):
    env = SimpleNamespace(kind=kind, auto_reset=auto_reset)
    return env, SimpleNamespace(obs_dim=13, n_actions=2), SimpleNamespace(obs_dim=16, n_actions=11)


def test_collector_argument_checks_need_no_handle():
    env, s, p = _fake()
    _check_modular(env, s, p, 4, 2024, 2025)
    for bad in (dict(env=_fake(kind="press")[0]), dict(env=_fake(auto_reset=False)[0]), dict(s=None), dict(p=None),
                dict(s=p), dict(p=s), dict(k=0), dict(seeds=(7, 7))):
        a = dict(env=env, s=s, p=p, k=4, seeds=(2024, 2025))
        a.update(bad)
        with pytest.raises(ValueError):
            _check_modular(a["env"], a["s"], a["p"], a["k"], *a["seeds"])


def test_trainer_argument_checks_need_no_handle():
    _, s, p = _fake()
    col = SimpleNamespace(sort_agent=s, press_agent=p)
    with pytest.raises(ValueError, match="at least one learner"):
        ModularTrainer(col)
    with pytest.raises(ValueError, match="reward"):
        ModularTrainer(col, sort_learner=SimpleNamespace(policy=s), reward="each")
    with pytest.raises(ValueError, match="sort_agent"):
        ModularTrainer(col, sort_learner=SimpleNamespace(policy=p))
    with pytest.raises(ValueError, match="press_agent"):
        ModularTrainer(col, press_learner=SimpleNamespace(policy=s))
    t = ModularTrainer(col, press_learner=SimpleNamespace(policy=p), reward="team")
    assert t.learners["sort"] is None and t.reward == "team"
    with pytest.raises(ValueError, match="first_iteration"):
        t.learn(2, first_iteration=5)


def test_buffer_struct_mirrors_the_header():
    text = open(os.path.join(ROOT, "include", "mse.h")).read()
    body = re.search(r"typedef struct mse_modular_buffers \{(.*?)\} mse_modular_buffers;", text, re.S).group(1)
    members = re.findall(r"(\w+)\s*\*?\s*(\w+);", body)
    assert [name for _, name in members] == ["struct_size", "reserved0", *_lib.MODULAR_BUFFER_NAMES]
    assert [name for name, _ in _lib.MseModularBuffers._fields_] == [name for _, name in members]
    assert C.sizeof(_lib.MseModularBuffers) == 8 + 8 * len(_lib.MODULAR_BUFFER_NAMES)
    # the element types of the header agree with the tensors the collectors allocate
    ctype = {"float": torch.float32, "int32_t": torch.int32, "uint8_t": torch.uint8}
    b = _modular_buffers(1, 1, "cpu")
    for typ, name in members[2:]:
        assert b[name].dtype == ctype[typ], name
    flags = dict(re.findall(r"#define (MSE_MODULAR_\w+)\s+(\d+)u", text))
    assert int(flags["MSE_MODULAR_SORT_DETERMINISTIC"]) == _lib.MSE_MODULAR_SORT_DETERMINISTIC
    assert int(flags["MSE_MODULAR_PRESS_DETERMINISTIC"]) == _lib.MSE_MODULAR_PRESS_DETERMINISTIC
