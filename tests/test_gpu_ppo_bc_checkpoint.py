"""GPU: a run with `bc_coef` resumes bit for bit, and its file is refused by name by a learner without it.  The run is
tests/checkpoint_checks.py's "two_launch" case with the collector labelling its rollouts (expert_labels=True) and a linear
bc_coef schedule or a constant; what is compared is that file's `final_state` plus `bc_coef`."""
import math

import pytest

from tests import checkpoint_checks as CC
from tests.checkpoint_checks import AT, ITERS

pytestmark = pytest.mark.gpu

CASE = "two_launch"


def _build(bc_coef, fresh=False):
    import marl_sortingenv_amd as M

    run = CC.build(CASE, fresh=fresh, learner_kw=None if bc_coef is None else dict(bc_coef=bc_coef))
    run["collector"] = M.PolicyRolloutCollector(run["env"], run["policy"], CC.K, seed=22, expert_labels=True)
    return run


def _state(run):
    return dict(CC.final_state(run), bc_coef=run["learner"].bc_coef)


def _same(a, b):
    from marl_sortingenv_amd.checkpoint import same_value

    return same_value(a, b)


@pytest.mark.parametrize("schedule", ["const", "linear"])
def test_a_resumed_run_with_bc_coef_is_the_straight_run(schedule, tmp_path):
    import marl_sortingenv_amd as M
    from marl_sortingenv_amd.checkpoint import read_checkpoint

    def coef():
        return 0.5 if schedule == "const" else (lambda p: 2.0 * p)

    run_a = _build(coef())
    rec_a = run_a["learner"].learn(run_a["collector"], ITERS, checkpoint_path=tmp_path / "straight_{iteration}.pt", checkpoint_freq=AT,
                                   **run_a["learn_kw"])
    state_a = _state(run_a)
    at2 = str(tmp_path / f"straight_{AT}.pt")
    ck2 = read_checkpoint(at2)
    hp = ck2["learner"]["hyperparameters"]
    if schedule == "const":
        assert hp["bc_coef"] == 0.5 and hp["scheduled"] == [] and ck2["learner"]["bc_coef"] == 0.5
        assert [r["bc_coef"] for r in rec_a] == [0.5] * ITERS
    else:
        assert "bc_coef" not in hp and hp["scheduled"] == ["bc_coef"] and ck2["learner"]["bc_coef"] == 2.0 * (1.0 - AT / ITERS)
        assert [r["bc_coef"] for r in rec_a] == [2.0 * (1.0 - (i + 1) / ITERS) for i in range(ITERS)] and rec_a[-1]["bc_coef"] == 0.0
    for r in rec_a:
        print(f"bc record: bc_coef {r['bc_coef']} bc_loss {r['bc_loss']:.4f} accuracy {r['bc_accuracy']:.4f} unusable {r['bc_unusable']:.4f}")
    assert all(r["bc_loss"] > 0.0 and 0.0 <= r["bc_unusable"] <= 1.0 and 0.0 <= r["bc_accuracy"] <= 1.0 for r in rec_a)

    run_b = _build(coef(), fresh=True)
    ck = M.load_checkpoint(at2, learner=run_b["learner"], collector=run_b["collector"])
    assert ck["iteration"] == AT and run_b["learner"].bc_coef == ck2["learner"]["bc_coef"]
    rec_b = run_b["learner"].learn(run_b["collector"], ITERS, first_iteration=ck["iteration"], history=ck["history"],
                                   checkpoint_path=tmp_path / "resumed_{iteration}.pt", checkpoint_freq=AT, **run_b["learn_kw"])
    state_b = _state(run_b)
    assert len(rec_a) == len(rec_b) == ITERS
    for a, b in zip(rec_a, rec_b):
        assert a.keys() == b.keys()
        for key in a:
            assert a[key] == b[key] or (isinstance(a[key], float) and math.isnan(a[key]) and math.isnan(b[key])), key
    assert state_a.keys() == state_b.keys()
    for key in state_a:
        assert _same(state_a[key], state_b[key]), key
    last_a, last_b = read_checkpoint(tmp_path / f"straight_{ITERS}.pt"), read_checkpoint(tmp_path / f"resumed_{ITERS}.pt")
    assert _same(last_a["learner"], last_b["learner"]) and _same(last_a["collector"], last_b["collector"])


def test_a_file_with_bc_coef_is_refused_by_name_by_a_learner_without_it(tmp_path):
    import marl_sortingenv_amd as M

    run = _build(0.5)
    run["learner"].learn(run["collector"], 1, checkpoint_path=tmp_path / "with.pt", checkpoint_freq=1, **run["learn_kw"])
    for other, named in ((None, "bc_coef"), (0.25, "bc_coef"), (lambda p: 0.5 * p, "bc_coef")):
        fresh = _build(other, fresh=True)
        before = fresh["learner"].weights.clone()
        with pytest.raises(ValueError, match=named):
            M.load_checkpoint(tmp_path / "with.pt", learner=fresh["learner"], collector=fresh["collector"])
        assert bool((fresh["learner"].weights == before).all())
    # ... and the other way round: a file without it, a learner with it
    plain = _build(None)
    plain["learner"].learn(plain["collector"], 1, checkpoint_path=tmp_path / "without.pt", checkpoint_freq=1, **plain["learn_kw"])
    with pytest.raises(ValueError, match="bc_coef"):
        fresh = _build(0.5, fresh=True)
        M.load_checkpoint(tmp_path / "without.pt", learner=fresh["learner"], collector=fresh["collector"])
