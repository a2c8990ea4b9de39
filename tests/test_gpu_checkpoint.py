"""GPU: a training run checkpointed after 2 of 4 iterations and resumed in fresh objects IS the run of 4 iterations
straight through - equality, not closeness - for every option of the learner that carries state, the three env kinds and
both collectors; the same resume in a fresh child process; what `load_checkpoint` refuses and that a refusal touches
nothing; `envs=False`; and that the file loads with `weights_only=True`.  The run is tests/checkpoint_checks.py's.

TARGET_KL was picked on the MI355X so that the straight run of the `target_kl` case stops inside updates after the
checkpoint (the figures are at its definition); the test asserts that, so the case cannot stop exercising the gate
unnoticed."""
import math
import os
import subprocess
import sys

import pytest

from tests import checkpoint_checks as CC
from tests.checkpoint_checks import AT, ITERS, N

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# Measured on an MI355X: the ungated run of the `target_kl` case reaches approx_kl 1.3e-4, 3.4e-4, 6.7e-4 and 1.6e-4 in the
# last minibatch of its four updates (SB3 stops above 1.5 * target_kl).  With 1e-4 the straight run's records read (stopped,
# minibatches_run) = (False, 6), (True, 5), (True, 4), (False, 6) and 19 of 24 Adam steps are taken: one update stops before
# the checkpoint, one after it, and one on either side runs to its end.  3e-5 .. 2e-4 all stop in iteration 2.
TARGET_KL = 1e-4


def _same(a, b):
    from marl_sortingenv_amd.checkpoint import same_value

    return same_value(a, b)


def _assert_same_tree(a, b, label):
    assert isinstance(a, dict) and isinstance(b, dict) and a.keys() == b.keys(), (label, sorted(a), sorted(b))
    for key in a:
        if isinstance(a[key], dict) and isinstance(b[key], dict):
            _assert_same_tree(a[key], b[key], f"{label}.{key}")
        else:
            assert _same(a[key], b[key]), f"{label}.{key}: {a[key]!r} != {b[key]!r}"


def _assert_same_records(a, b, label):
    assert len(a) == len(b) == ITERS, label
    for i in range(ITERS):
        assert a[i].keys() == b[i].keys(), (label, i)
        for key in a[i]:
            x, y = a[i][key], b[i][key]
            assert type(x) is type(y), (label, i, key)
            assert x == y or (isinstance(x, float) and math.isnan(x) and math.isnan(y)), (label, i, key, x, y)


def _straight(case, tmp_path, target_kl=None):
    """The run of 4 iterations with a checkpoint after every 2nd -> (run, records, final state, the two files)."""
    run = CC.build(case, target_kl=target_kl)
    pattern = tmp_path / "straight_{iteration}.pt"
    records = run["learner"].learn(run["collector"], ITERS, checkpoint_path=pattern, checkpoint_freq=AT, **run["learn_kw"])
    files = [str(tmp_path / f"straight_{i}.pt") for i in (AT, ITERS)]
    assert all(os.path.exists(f) for f in files) and len(os.listdir(tmp_path)) == 2
    return run, records, CC.final_state(run), files


# ---- 1. straight against resumed, in one process ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CC.CASES))
def test_a_resumed_run_is_the_straight_run(case, tmp_path):
    from marl_sortingenv_amd.checkpoint import read_checkpoint

    target_kl = TARGET_KL if case == "target_kl" else None
    run_a, rec_a, state_a, (at2, at4) = _straight(case, tmp_path, target_kl)
    ck2 = read_checkpoint(at2)
    assert ck2["iteration"] == AT and ck2["iterations"] == ITERS and len(ck2["history"]) == AT
    assert sorted(k for k in ck2 if k in ("learner", "collector", "policies")) == \
        ["collector", "learner"] + (["policies"] if case == "press" else [])
    if case == "target_kl":
        for rec in rec_a:
            print("target_kl record:", rec["stopped"], rec["minibatches_run"], rec["approx_kl"])
        assert any(rec["stopped"] for rec in rec_a[AT:]), "the gate must close at least once after the checkpoint"
        assert run_a["learner"].step < ITERS * CC.EPOCHS * 3
    if "episode_stats" in CC.CASES[case][3]:
        for rec in rec_a:
            print("episode record:", rec["episodes"], rec["ep_rew_mean"], rec["ep_len_mean"])
        # Episodes end on steps 12 and 24 (no env overflows in this run): records 1 and 2 close 96 episodes each, record 3
        # (steps 25 .. 32) closes none whatever the code does - measured 0 / 96 / 96 / 0.  So the episodes that must come out
        # right are record 2's: each is 4 steps before the checkpoint and 8 after it, and its length is 12 only with the
        # carry restored.  Record 3's open episodes (8 steps each) are held equal through the iteration-4 files below.
        assert rec_a[2]["episodes"] > 0 and rec_a[2]["ep_len_mean"] == CC.MAX_STEPS
        run_length = ck2["learner"]["episode_stats"]["run_length"]
        assert bool((run_length != 0).all()) and bool((ck2["learner"]["episode_stats"]["run_return"] != 0).any()), \
            "the carry must matter at the checkpoint"
    if case == "eval":
        assert all("eval_mean_reward" in r for r in rec_a) and "best_weights" in ck2["learner"]
        assert math.isfinite(ck2["learner"]["best_mean_reward"])
    if case == "schedules":
        assert [r["learning_rate"] for r in rec_a] == [CC.LR * (1.0 - (i + 1) / ITERS) for i in range(ITERS)]
        assert ck2["learner"]["hyperparameters"]["scheduled"] == ["clip_range", "learning_rate"]
        assert ck2["learner"]["progress_remaining"] == 0.5 and all("explained_variance" in r for r in rec_a)
    if case == "press":
        assert ck2["policies"]["sort_policy"]["obs_dim"] == 13

    run_b, rec_b, state_b = CC.resume(case, at2, tmp_path / "resumed_{iteration}.pt", target_kl)
    assert _same(rec_b[:AT], ck2["history"])
    _assert_same_records(rec_a, rec_b, case)
    _assert_same_tree(state_a, state_b, case)
    if case == "eval":
        assert "restored_best_weights" in state_a and state_a["best_mean_reward"] == state_b["best_mean_reward"]
    _assert_same_tree(read_checkpoint(at4), read_checkpoint(tmp_path / f"resumed_{ITERS}.pt"), f"{case} file")


# ---- 2. the same resume in a fresh child process ------------------------------------------------------------------------------
def test_a_run_resumed_in_a_child_process_is_the_straight_run(tmp_path):
    from marl_sortingenv_amd.checkpoint import read_checkpoint

    case = "device-device"
    run_a, rec_a, state_a, (at2, at4) = _straight(case, tmp_path)
    out = str(tmp_path / "child.pt")
    done = subprocess.run([sys.executable, "-m", "tests.checkpoint_checks", case, at2, out], cwd=ROOT, timeout=120,
                          capture_output=True, text=True)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
    child = read_checkpoint(out)
    _assert_same_records(rec_a, child["history"], "child")
    _assert_same_tree(state_a, child["extra"], "child")
    _assert_same_tree(read_checkpoint(at4), read_checkpoint(out + ".last"), "child file")


# ---- 3. - 5. refusals, envs=False, load safety: one mono file for all ---------------------------------------------------------
@pytest.fixture(scope="module")
def mono_file(tmp_path_factory):
    d = tmp_path_factory.mktemp("ck")
    run = CC.build("cpu-host")
    run["learner"].learn(run["collector"], AT, checkpoint_path=d / "mono_{iteration}.pt", checkpoint_freq=AT)
    import marl_sortingenv_amd as M

    M.save_checkpoint(d / "mono_noenvs.pt", learner=run["learner"], collector=run["collector"], iteration=AT, iterations=ITERS,
                      envs=False)
    return str(d / f"mono_{AT}.pt"), str(d / "mono_noenvs.pt")


def _snapshot(run):
    import torch

    torch.cuda.synchronize()
    lrn, env = run["learner"], run["env"]
    snap = {name: getattr(lrn, name).clone() for name in ("weights", "m", "v")}
    snap.update(zip(("ints", "dbls", "rng"), (t.clone() for t in env.get_state())))
    snap.update(step=lrn.step, epochs_done=lrn.epochs_done, generator=lrn.generator.get_state().clone(),
                policy_step=env.policy_step, image=CC.image(run["policy"]), obs=env.obs.clone(), mask=env.mask.clone(),
                n_epochs=lrn.n_epochs, learning_rate=lrn.learning_rate, progress_remaining=lrn.progress_remaining)
    return snap


def _assert_untouched(run, snap, label):
    now = _snapshot(run)
    for key in snap:
        a, b = snap[key], now[key]
        assert _same(a.cpu() if hasattr(a, "cpu") else a, b.cpu() if hasattr(b, "cpu") else b), (label, key)


@pytest.mark.parametrize("label, build_kw, field", [
    ("a mono file into a press env", dict(kind="press"), "kind"),
    ("96 envs into 97", dict(num_envs=N + 1), "num_envs"),
    ("another max_steps", dict(max_steps=CC.MAX_STEPS + 1), "max_steps"),
])
def test_an_env_of_another_fingerprint_is_refused_untouched(mono_file, label, build_kw, field):
    import marl_sortingenv_amd as M
    from marl_sortingenv_amd.checkpoint import read_checkpoint

    run = CC.build("cpu-host", fresh=True, **build_kw)
    snap = _snapshot(run)
    learner = None if "kind" in build_kw else run["learner"]  # other dims: the learner has a case of its own
    for strict in (True, False):
        with pytest.raises(ValueError) as e:
            M.load_checkpoint(mono_file[0], learner=learner, collector=run["collector"], strict=strict)
        assert field in str(e.value) and "checkpoint has" in str(e.value), str(e.value)
        _assert_untouched(run, snap, (label, strict))
    if field == "kind":
        assert "'mono'" in str(e.value) and "'press'" in str(e.value)
    if field == "max_steps":
        assert "config.max_steps" in str(e.value) and "config.noise" not in str(e.value)
    if field == "num_envs":
        assert f"checkpoint has {N}, this object has {N + 1}" in str(e.value)
    with pytest.raises(ValueError, match=field):
        run["env"].load_state_dict(read_checkpoint(mono_file[0])["collector"]["env"])
    _assert_untouched(run, snap, (label, "env"))


def test_a_learner_of_other_hyperparameters_is_refused_only_when_strict(mono_file):
    import marl_sortingenv_amd as M
    from marl_sortingenv_amd.checkpoint import read_checkpoint

    run = CC.build("cpu-host", fresh=True, learner_kw=dict(n_epochs=CC.EPOCHS + 1, learning_rate=5e-4))
    snap = _snapshot(run)
    with pytest.raises(ValueError) as e:
        M.load_checkpoint(mono_file[0], learner=run["learner"], collector=run["collector"])
    msg = str(e.value)
    assert f"n_epochs: checkpoint has {CC.EPOCHS}, this object has {CC.EPOCHS + 1}" in msg
    assert f"learning_rate: checkpoint has {CC.LR!r}, this object has 0.0005" in msg and "gamma" not in msg
    _assert_untouched(run, snap, "strict")
    out = M.load_checkpoint(mono_file[0], learner=run["learner"], collector=run["collector"], strict=False)
    assert out["loaded"] == ["collector", "learner"] and out["iteration"] == AT
    sd = read_checkpoint(mono_file[0])["learner"]
    lrn = run["learner"]
    assert lrn.n_epochs == CC.EPOCHS + 1 and lrn.learning_rate == 5e-4  # the constructor's values are kept
    assert _same(lrn.weights.cpu(), sd["weights"]) and _same(lrn.m.cpu(), sd["m"]) and _same(lrn.v.cpu(), sd["v"])
    assert lrn.step == sd["step"] and _same(lrn.generator.get_state(), sd["generator"])
    assert _same(run["policy"].flat_weights().tolist(), sd["weights"].tolist())
    lrn.learn(run["collector"], ITERS, first_iteration=AT)  # and it trains on, 3 epochs a time
    assert lrn.step == sd["step"] + (ITERS - AT) * (CC.EPOCHS + 1) * 3


def test_a_learner_of_other_dims_is_always_refused(mono_file):
    import marl_sortingenv_amd as M

    run = CC.build("press", fresh=True)
    snap = _snapshot(run)
    for strict in (True, False):
        with pytest.raises(ValueError) as e:
            M.load_checkpoint(mono_file[0], learner=run["learner"], strict=strict)
        assert "obs_dim: checkpoint has 29, this object has 16" in str(e.value) and "n_actions" in str(e.value)
        _assert_untouched(run, snap, strict)


@pytest.mark.parametrize("side", ["learner", "file"])
def test_a_field_scheduled_on_one_side_only_is_refused(mono_file, side, tmp_path):
    import marl_sortingenv_amd as M

    if side == "learner":  # a scheduled learner, a file without schedules
        path, run = mono_file[0], CC.build("schedules", fresh=True)
    else:
        made = CC.build("schedules")
        path = str(tmp_path / "scheduled.pt")
        M.save_checkpoint(path, learner=made["learner"], collector=made["collector"])
        run = CC.build("cpu-host", fresh=True, learner_kw=dict(clip_range_vf=0.2))
    snap = _snapshot(run)
    with pytest.raises(ValueError) as e:
        M.load_checkpoint(path, learner=run["learner"], collector=run["collector"])
    assert "scheduled" in str(e.value) and "learning_rate" in str(e.value) and "<absent>" in str(e.value), str(e.value)
    _assert_untouched(run, snap, side)


def test_a_handle_with_a_trace_attached_refuses_both_calls(mono_file):
    from marl_sortingenv_amd.checkpoint import read_checkpoint

    run = CC.build("cpu-host", fresh=True)
    sd = read_checkpoint(mono_file[0])["collector"]["env"]
    run["env"].trace_begin(0, capacity=16)
    snap = _snapshot(run)
    with pytest.raises(RuntimeError, match="trace"):
        run["env"].state_dict()
    with pytest.raises(RuntimeError, match="trace"):
        run["env"].load_state_dict(sd)
    _assert_untouched(run, snap, "trace")
    run["env"].trace_end()
    run["env"].load_state_dict(sd)
    assert _same(run["env"].state_dict()["rng"], sd["rng"])


def test_a_file_without_envs_has_no_env_section_and_loads_only_when_not_strict(mono_file):
    import marl_sortingenv_amd as M
    from marl_sortingenv_amd.checkpoint import read_checkpoint

    tree = read_checkpoint(mono_file[1])
    assert "collector" not in tree and "learner" in tree
    run = CC.build("cpu-host", fresh=True)
    snap = _snapshot(run)
    with pytest.raises(ValueError, match="collector"):
        M.load_checkpoint(mono_file[1], learner=run["learner"], collector=run["collector"])
    _assert_untouched(run, snap, "strict")
    out = M.load_checkpoint(mono_file[1], learner=run["learner"], collector=run["collector"], strict=False)
    assert out["loaded"] == ["learner"]
    for key in ("ints", "dbls", "rng", "policy_step", "obs", "mask"):  # the env is as it was
        now = _snapshot(run)
        assert _same(snap[key].cpu() if hasattr(snap[key], "cpu") else snap[key],
                     now[key].cpu() if hasattr(now[key], "cpu") else now[key]), key
    assert _same(run["learner"].weights.cpu(), tree["learner"]["weights"]) and run["learner"].step == tree["learner"]["step"]


def test_the_file_loads_with_weights_only_and_holds_plain_data(mono_file):
    import torch

    from marl_sortingenv_amd.checkpoint import FORMAT_VERSION, validate_tree

    for path in mono_file:
        tree = torch.load(path, map_location="cpu", weights_only=True)
        validate_tree(tree)
        assert tree["format_version"] == FORMAT_VERSION and tree["mse_version"] == 200
    env = torch.load(mono_file[0], map_location="cpu", weights_only=True)["collector"]["env"]
    assert env["ints"].shape[0] == N and env["policy_step"] == AT * CC.K and env["fingerprint"]["config"].dtype == torch.uint8
    per_env = sum(env[k].numel() * env[k].element_size() for k in ("ints", "dbls", "rng")) // N
    assert per_env == 840
