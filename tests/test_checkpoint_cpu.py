"""CPU: the pure-host parts of marl_sortingenv_amd.checkpoint on hand-built trees - what may be in a checkpoint, the
atomic write, the format version, the fingerprint comparison and its message, the CPU generator's round trip and the
`{iteration}` field of a path.  No device is touched."""
import os

import pytest
import torch

from marl_sortingenv_amd import checkpoint as CK


def _tree(**extra):
    t = {"format_version": CK.FORMAT_VERSION, "mse_version": 200, "iteration": 2, "iterations": 4,
         "history": [{"loss": 0.5, "reward": float("nan"), "stopped": False, "minibatches_run": 6}], "extra": None,
         "learner": {"weights": torch.arange(5, dtype=torch.float32), "step": 12, "best_mean_reward": float("-inf"),
                     "hyperparameters": {"shuffle": "cpu", "target_kl": None, "scheduled": ["clip_range", "learning_rate"]}}}
    t.update(extra)
    return t


class _Thing:
    pass


# ---- what may be in a checkpoint ----------------------------------------------------------------------------------------
def test_a_tree_of_tensors_and_plain_containers_is_accepted():
    CK.validate_tree(_tree())
    CK.validate_tree({"a": (1, 2.0, "x", True, None), 3: [torch.zeros(2, dtype=torch.uint8)]})


@pytest.mark.parametrize("bad, where", [
    (lambda p: 3e-4 * p, "['learner']['schedule']"),
    (_Thing(), "['learner']['schedule']"),
    ({1, 2}, "['learner']['schedule']"),
    (torch.Generator(), "['learner']['schedule']"),
])
def test_a_callable_or_an_object_is_refused_and_named(bad, where):
    t = _tree()
    t["learner"]["schedule"] = bad
    with pytest.raises(TypeError) as e:
        CK.validate_tree(t)
    assert where in str(e.value) and type(bad).__name__ in str(e.value)


def test_odd_keys_and_container_subclasses_are_refused():
    import collections

    with pytest.raises(TypeError, match="keys"):
        CK.validate_tree({(1, 2): 0})
    with pytest.raises(TypeError, match="keys"):
        CK.validate_tree({True: 0})
    with pytest.raises(TypeError, match="defaultdict"):
        CK.validate_tree({"a": collections.defaultdict(list)})


def test_a_refused_tree_is_refused_before_anything_is_written(tmp_path):
    path = tmp_path / "run.pt"
    t = _tree()
    t["history"].append({"callback": print})
    with pytest.raises(TypeError, match="history"):
        CK.atomic_save(t, path)
    assert os.listdir(tmp_path) == []


# ---- the atomic write ---------------------------------------------------------------------------------------------------
def test_atomic_save_writes_a_file_that_loads_with_weights_only(tmp_path):
    path = tmp_path / "run.pt"
    assert CK.atomic_save(_tree(), path) == str(path)
    assert os.listdir(tmp_path) == ["run.pt"]
    back = torch.load(path, map_location="cpu", weights_only=True)
    assert CK.same_value(back, _tree())
    assert CK.same_value(CK.read_checkpoint(path), _tree())


def test_atomic_save_keeps_the_previous_file_when_serialisation_fails_half_way(tmp_path):
    path = tmp_path / "run.pt"
    CK.atomic_save(_tree(iteration=2), path)
    before = path.read_bytes()

    def half_way(tree, f):
        f.write(b"half a checkpoint")
        f.flush()
        raise OSError("disk full")

    with pytest.raises(OSError, match="disk full"):
        CK.atomic_save(_tree(iteration=4), path, serializer=half_way)
    assert path.read_bytes() == before
    assert os.listdir(tmp_path) == ["run.pt"]  # the temporary file is gone
    assert CK.read_checkpoint(path)["iteration"] == 2
    CK.atomic_save(_tree(iteration=4), path)
    assert CK.read_checkpoint(path)["iteration"] == 4


def test_atomic_save_into_a_missing_directory_fails_without_side_effects(tmp_path):
    with pytest.raises(OSError):
        CK.atomic_save(_tree(), tmp_path / "nowhere" / "run.pt")
    assert os.listdir(tmp_path) == []


# ---- the format version -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("version", [0, CK.FORMAT_VERSION + 1, None, "1", 1.0, True])
def test_an_unknown_format_version_is_refused(version, tmp_path):
    with pytest.raises(ValueError, match="format version"):
        CK.check_format_version(version)
    path = tmp_path / "other.pt"
    torch.save(_tree(format_version=version), path)
    with pytest.raises(ValueError, match="format version"):
        CK.read_checkpoint(path)
    with pytest.raises(ValueError, match="format version"):
        CK.load_checkpoint(path)


def test_the_current_format_version_is_accepted():
    CK.check_format_version(CK.FORMAT_VERSION)


def test_load_checkpoint_without_objects_returns_the_rest(tmp_path):
    path = tmp_path / "run.pt"
    CK.atomic_save(_tree(extra={"note": "stage 1"}), path)
    out = CK.load_checkpoint(path)
    assert out["iteration"] == 2 and out["iterations"] == 4 and out["extra"] == {"note": "stage 1"}
    assert out["format_version"] == CK.FORMAT_VERSION and out["mse_version"] == 200 and out["loaded"] == []
    assert CK.same_value(out["history"], _tree()["history"])


def test_missing_sections_lists_what_is_asked_for_and_absent():
    t = _tree(policies={"sort_policy": {}})
    assert CK.missing_sections(t) == []
    assert CK.missing_sections(t, learner=object()) == []
    assert CK.missing_sections(t, learner=object(), collector=object()) == ["collector"]
    assert CK.missing_sections(t, policies={"sort_policy": 1, "press": 2}) == ["policies['press']"]


# ---- fingerprints -------------------------------------------------------------------------------------------------------
def test_fingerprint_comparison_names_every_differing_field_with_both_values():
    saved = {"kind": "mono", "num_envs": 96, "max_steps": 12, "auto_reset": True, "config": torch.arange(8, dtype=torch.uint8),
             "target_kl": None, "nan": float("nan")}
    mine = dict(saved, kind="press", num_envs=97, config=torch.arange(8, dtype=torch.uint8), nan=float("nan"))
    assert CK.diff_fields(saved, saved) == []
    assert [d[0] for d in CK.diff_fields(saved, mine)] == ["kind", "num_envs"]
    with pytest.raises(ValueError) as e:
        CK.check_fingerprint(saved, mine, "BatchedSortingEnv")
    msg = str(e.value)
    assert "BatchedSortingEnv" in msg and "kind: checkpoint has 'mono', this object has 'press'" in msg
    assert "num_envs: checkpoint has 96, this object has 97" in msg and "max_steps" not in msg and "config" not in msg
    CK.check_fingerprint(saved, dict(saved), "BatchedSortingEnv")


def test_fingerprint_comparison_sees_tensors_absent_fields_and_types():
    saved = {"config": torch.arange(8, dtype=torch.uint8), "scheduled": ["learning_rate"], "learning_rate": 3e-4, "flag": True}
    other = torch.arange(8, dtype=torch.uint8)
    other[5] = 0
    mine = {"config": other, "scheduled": [], "flag": 1, "clip_range": 0.2}
    names = [d[0] for d in CK.diff_fields(saved, mine)]
    assert names == ["clip_range", "config", "flag", "learning_rate", "scheduled"]
    msg = CK.mismatch_message("PPOLearner", CK.diff_fields(saved, mine))
    assert "learning_rate: checkpoint has 0.0003, this object has '<absent>'" in msg
    assert "clip_range: checkpoint has '<absent>', this object has 0.2" in msg and "<uint8[8]>" in msg
    # only the fields asked for
    assert [d[0] for d in CK.diff_fields(saved, mine, fields=("config", "nothing"))] == ["config"]
    assert not CK.same_value(torch.zeros(2), torch.zeros(2, dtype=torch.float64)) and not CK.same_value(torch.zeros(2), [0.0, 0.0])


# ---- the CPU generator --------------------------------------------------------------------------------------------------
def test_the_cpu_generators_state_round_trips_through_a_file(tmp_path):
    g = torch.Generator(device="cpu").manual_seed(5)
    torch.randperm(768, generator=g)
    path = tmp_path / "g.pt"
    CK.atomic_save({"format_version": CK.FORMAT_VERSION, "generator": CK.generator_state(g)}, path)
    want = [torch.randperm(768, generator=g) for _ in range(2)]
    fresh = torch.Generator(device="cpu").manual_seed(99)
    state = CK.read_checkpoint(path)["generator"]
    assert state.dtype == torch.uint8
    CK.set_generator_state(fresh, state)
    got = [torch.randperm(768, generator=fresh) for _ in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(want, got))
    assert not torch.equal(want[0], torch.randperm(768, generator=torch.Generator(device="cpu").manual_seed(99)))


def test_generator_state_is_a_copy():
    g = torch.Generator(device="cpu").manual_seed(1)
    s = CK.generator_state(g)
    keep = s.clone()
    torch.randperm(10, generator=g)
    assert torch.equal(s, keep) and not torch.equal(g.get_state(), keep)


# ---- paths ----------------------------------------------------------------------------------------------------------------
def test_the_iteration_field_of_a_path_is_formatted(tmp_path):
    assert CK.format_path("run.pt", 7) == "run.pt"
    assert CK.format_path("run_{iteration}.pt", 7) == "run_7.pt"
    assert CK.format_path("run_{iteration:04d}.pt", 7) == "run_0007.pt"
    assert CK.format_path(tmp_path / "ck_{iteration}.pt", 12) == str(tmp_path / "ck_12.pt")


def test_the_package_exports_save_and_load():
    import marl_sortingenv_amd as M

    assert M.save_checkpoint is CK.save_checkpoint and M.load_checkpoint is CK.load_checkpoint
    assert "save_checkpoint" in M.__all__ and "load_checkpoint" in M.__all__
