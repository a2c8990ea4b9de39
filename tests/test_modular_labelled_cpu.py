"""CPU: the host-only side of the labelled modular collection - the ctypes mirror of struct mse_modular_label_buffers
against include/mse.h, the check-only entry point without a device, the key sets of view() / demo_view() with and without
labels, and the argument rules that need no handle (beta, the mixture seed)."""
import ctypes as C
import math
import os
import re
from types import SimpleNamespace

import pytest
import torch

import marl_sortingenv_amd as M
from marl_sortingenv_amd import _lib
from marl_sortingenv_amd.collector import (_ModularBase, _modular_buffers, _modular_label_buffers, demo_view, modular_mix_seed,
                                           modular_view)
from marl_sortingenv_amd.modular import ModularTrainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIEW_KEYS = {"observations", "action_masks", "actions", "log_probs", "values", "rewards", "episode_starts", "last_values",
             "last_dones"}
DEMO_KEYS = {"observations", "action_masks", "actions", "stepped_actions", "expert_stepped", "rewards", "episode_starts",
             "last_dones", "returns"}


def test_label_struct_mirrors_the_header():
    text = open(os.path.join(ROOT, "include", "mse.h")).read()
    body = re.search(r"typedef struct mse_modular_label_buffers \{(.*?)\} mse_modular_label_buffers;", text, re.S).group(1)
    members = re.findall(r"(\w+)\s*\*?\s*(\w+);", body)
    assert [name for _, name in members] == ["struct_size", "reserved0", *_lib.MODULAR_LABEL_BUFFER_NAMES]
    assert [name for name, _ in _lib.MseModularLabelBuffers._fields_] == [name for _, name in members]
    assert [typ for typ, _ in members[:2]] == ["uint32_t", "uint32_t"]
    assert C.sizeof(_lib.MseModularLabelBuffers) == 8 + 8 * 4 == 40
    assert _lib.MseModularLabelBuffers.sort_expert_actions.offset == 8 and _lib.MseModularLabelBuffers.expert_stepped.offset == 32
    ctype = {"float": torch.float32, "int32_t": torch.int32, "uint8_t": torch.uint8}
    b = _modular_label_buffers(1, 1, "cpu")
    assert tuple(b) == _lib.MODULAR_LABEL_BUFFER_NAMES
    for typ, name in members[2:]:
        assert b[name].dtype == ctype[typ] and tuple(b[name].shape) == (1, 1), name
    # mse_modular_buffers did not change: its size is an ABI check
    assert C.sizeof(_lib.MseModularBuffers) == 8 + 8 * 16
    # both entry points are declared with the arguments the binding passes
    for name, n_args in (("mse_rollout_modular_labelled", 12), ("mse_rollout_modular_labelled_check", 9)):
        decl = re.search(r"\bint " + name + r"\((.*?)\);", text, re.S).group(1)
        assert len(decl.split(",")) == n_args and name in _lib.EXPORTS, name


def test_check_entry_refuses_a_null_env_without_a_device():
    L = M.load_library()
    assert len(L.mse_rollout_modular_labelled_check.argtypes) == 9 and len(L.mse_rollout_modular_labelled.argtypes) == 12
    assert L.mse_rollout_modular_labelled_check(None, None, None, 4, 1, 2, 3, 0, 0) == -1
    assert b"NULL" in L.mse_last_error()
    out, labels = _lib.MseModularBuffers(C.sizeof(_lib.MseModularBuffers), 0), _lib.MseModularLabelBuffers(40, 0)
    assert L.mse_rollout_modular_labelled(None, None, None, 4, 1, 2, 3, 0, 0, C.byref(out), C.byref(labels), None) == -1


def test_view_key_sets_with_and_without_labels():
    plain = _modular_buffers(5, 3, "cpu")
    assert set(plain) == set(_lib.MODULAR_BUFFER_NAMES)
    for who in ("sort", "press"):
        assert set(modular_view(plain, who)) == VIEW_KEYS
        with pytest.raises(KeyError, match="demo_view"):
            demo_view(plain, who)
    for returns in (False, True):
        b = dict(plain, **_modular_label_buffers(5, 3, "cpu", returns=returns))
        assert set(b) == set(_lib.MODULAR_BUFFER_NAMES) | set(_lib.MODULAR_LABEL_BUFFER_NAMES) | ({"returns"} if returns else set())
        for who in ("sort", "press"):
            v = modular_view(b, who, "team")
            assert set(v) == VIEW_KEYS | {"expert_actions"}
            assert v["expert_actions"] is b[f"{who}_expert_actions"] and v["actions"] is b[f"{who}_actions"]
            d = demo_view(b, who)
            assert set(d) == DEMO_KEYS
            assert d["observations"] is b[f"{who}_obs"] and d["actions"] is b[f"{who}_expert_actions"]
            assert d["stepped_actions"] is b["stepped_actions"] and d["expert_stepped"] is b["expert_stepped"]
            assert d["rewards"] is b["rewards"] and d["episode_starts"] is b["episode_starts"] and d["last_dones"] is b["last_dones"]
            assert (d["returns"] is b["returns"]) if returns else (d["returns"] is None)
        assert demo_view(b, "sort")["action_masks"] is None and demo_view(b, "press")["action_masks"] is b["press_masks"]
        assert demo_view(b, "press", press_masked=False)["action_masks"] is None
    with pytest.raises(ValueError, match="who"):
        demo_view(b, "presser")


def test_beta_and_seed_rules_need_no_handle():
    assert modular_mix_seed(2024, 2025) not in (2024, 2025) and modular_mix_seed(9, 3) not in (9, 3)
    assert modular_mix_seed(2024, 2025, 7) == 7
    for clash in (2024, 2025):
        with pytest.raises(ValueError, match="mix_seed"):
            modular_mix_seed(2024, 2025, clash)
    labelled, plain = _ModularBase.__new__(_ModularBase), _ModularBase.__new__(_ModularBase)
    labelled.expert_labels, plain.expert_labels = True, False
    for good in (0.0, 0.25, 1.0, 1):
        labelled.beta = good
        assert labelled.beta == float(good) and labelled._threshold == M.expert_threshold(good)
    assert labelled._threshold == 1 << 24
    for bad in (-0.01, 1.01, math.nan, math.inf):
        with pytest.raises(ValueError, match="beta"):
            labelled.beta = bad
        assert labelled.beta == 1.0
    plain.beta = 0.0
    for bad in (0.5, 1.0, math.nan):
        with pytest.raises(ValueError, match="beta"):
            plain.beta = bad
    assert plain.beta == 0.0 and plain._threshold == 0


def test_trainer_rules_need_no_handle():
    s, p = SimpleNamespace(obs_dim=13, n_actions=2), SimpleNamespace(obs_dim=16, n_actions=11)
    il = M.ImitationLearner.__new__(M.ImitationLearner)
    il.policy = s
    with pytest.raises(ValueError, match="expert_labels"):
        ModularTrainer(SimpleNamespace(sort_agent=s, press_agent=p), sort_learner=il)
    with pytest.raises(ValueError, match="expert_labels"):
        ModularTrainer(SimpleNamespace(sort_agent=s, press_agent=p, expert_labels=False), sort_learner=il)
    col = SimpleNamespace(sort_agent=s, press_agent=p, expert_labels=True)
    t = ModularTrainer(col, sort_learner=il, press_learner=SimpleNamespace(policy=p))
    assert t._on_policy_only() == ["press"]
    assert ModularTrainer(col, sort_learner=il)._on_policy_only() == []
    with pytest.raises(ValueError, match="expert_labels"):
        ModularTrainer(SimpleNamespace(sort_agent=s, press_agent=p), press_learner=SimpleNamespace(policy=p)).learn(1, beta=0.5)
