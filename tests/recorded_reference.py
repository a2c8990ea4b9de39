"""The reference's side of the oracle-vs-reference checks, recorded once and played back.

The checks in tests/test_oracle_vs_reference.py and tests/test_oracle_config_fuzz.py drive a reference env and the
oracle through the same script and compare them call by call.  `Recorder` wraps a live reference env (only where the
reference checkout is importable: `python -m oracle.gen_golden --vs-reference`) and notes what every call returned;
`Playback` answers the same calls from the stored fixture (tests/golden/recorded_reference_*.npz), so the checks run
anywhere.  Playback also asserts that the test asks what the recording was asked (seeds, actions, sorting modes,
keyword arguments): a script that drifted from the recording fails instead of comparing against the wrong rows.
"""
from __future__ import annotations

import json
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# one fixture per test module; a case's arrays are stored as "<case>__<field>"
FIXTURES = {
    "random_scripts": os.path.join(GOLDEN_DIR, "recorded_reference_random_scripts.npz"),
    "config_fuzz": os.path.join(GOLDEN_DIR, "recorded_reference_config_fuzz.npz"),
}

_FIELDS = ("reset_seed", "reset_obs", "mask", "step_args", "step_obs", "step_reward", "step_term", "step_info_action",
           "snap_ints", "snap_dbls", "snap_rng")
_loaded: dict = {}


def _kwargs_key(kwargs) -> str:
    return json.dumps({k: kwargs[k] for k in sorted(kwargs)}, sort_keys=True)


class Recorder:
    """A live reference env that notes what every call returned (fixture generation only)."""

    def __init__(self, env):
        self.env, self.agent = env, None
        self.rows = {k: [] for k in _FIELDS}
        self.step_kwargs: list[str] = []

    def set_agents(self, sort_agent=None):
        self.agent = sort_agent
        self.env.set_agents(sort_agent=sort_agent)

    def reset(self, seed=None):
        obs, info = self.env.reset(seed=seed)
        self.rows["reset_seed"].append(int(seed))
        self.rows["reset_obs"].append(np.asarray(obs, dtype=np.float32))
        return obs, info

    def action_masks(self):
        m = np.asarray(self.env.action_masks(), dtype=np.uint8)
        self.rows["mask"].append(m)
        return m

    def step(self, action=None, **kwargs):
        obs, rew, term, trunc, info = self.env.step(action, **kwargs)
        sm = -1 if self.agent is None else int(self.agent.next_mode)
        self.rows["step_args"].append((-1 if action is None else int(action), sm))
        self.step_kwargs.append(_kwargs_key(kwargs))
        self.rows["step_obs"].append(np.asarray(obs, dtype=np.float32))
        self.rows["step_reward"].append(float(rew))
        self.rows["step_term"].append(int(bool(term)))
        self.rows["step_info_action"].append(int(info["action"]) if isinstance(info, dict) and "action" in info else -1)
        return obs, rew, term, trunc, info

    def snapshot(self):
        from oracle import ref_harness

        I, D, R = ref_harness.snapshot(self.env)
        self.rows["snap_ints"].append(I)
        self.rows["snap_dbls"].append(D)
        self.rows["snap_rng"].append(R)
        return I, D, R

    def finish(self):
        pass

    def arrays(self, case: str) -> dict:
        dtypes = {"reset_seed": np.int64, "reset_obs": np.float32, "mask": np.uint8, "step_args": np.int64,
                  "step_obs": np.float32, "step_reward": np.float64, "step_term": np.uint8, "step_info_action": np.int64,
                  "snap_ints": np.int64, "snap_dbls": np.float64, "snap_rng": np.uint64}
        out = {f"{case}__{k}": np.asarray(v, dtype=dtypes[k]) for k, v in self.rows.items()}
        out[f"{case}__step_kwargs"] = np.frombuffer(json.dumps(self.step_kwargs).encode(), dtype=np.uint8)
        return out


class Playback:
    """Answers a test's calls on the reference env from the recorded fixture, in order."""

    def __init__(self, module: str, case: str):
        if module not in _loaded:
            with np.load(FIXTURES[module], allow_pickle=False) as z:
                _loaded[module] = {k: z[k] for k in z.files}
        z = _loaded[module]
        if f"{case}__reset_seed" not in z:
            raise KeyError(f"{FIXTURES[module]} holds no recording of {case!r} (python -m oracle.gen_golden --vs-reference)")
        self.case = case
        self.z = {k: z[f"{case}__{k}"] for k in _FIELDS}
        self.step_kwargs = json.loads(bytes(z[f"{case}__step_kwargs"]).decode())
        self.at = {k: 0 for k in ("reset", "mask", "step", "snap")}
        self.agent = None

    def _next(self, what: str) -> int:
        i = self.at[what]
        self.at[what] = i + 1
        return i

    def set_agents(self, sort_agent=None):
        self.agent = sort_agent

    def reset(self, seed=None):
        i = self._next("reset")
        assert int(seed) == int(self.z["reset_seed"][i]), f"{self.case}: reset #{i} seed {seed}, recorded {self.z['reset_seed'][i]}"
        return self.z["reset_obs"][i].copy(), {}

    def action_masks(self):
        return self.z["mask"][self._next("mask")].copy()

    def step(self, action=None, **kwargs):
        i = self._next("step")
        sm = -1 if self.agent is None else int(self.agent.next_mode)
        got = (-1 if action is None else int(action), sm)
        exp = tuple(int(x) for x in self.z["step_args"][i])
        assert got == exp, f"{self.case}: step #{i} asked (action, sort mode) {got}, recorded {exp}"
        assert _kwargs_key(kwargs) == self.step_kwargs[i], f"{self.case}: step #{i} kwargs {kwargs}, recorded {self.step_kwargs[i]}"
        info = {}
        if int(self.z["step_info_action"][i]) >= 0:
            info["action"] = int(self.z["step_info_action"][i])
        return (self.z["step_obs"][i].copy(), float(self.z["step_reward"][i]), bool(self.z["step_term"][i]), False, info)

    def snapshot(self):
        i = self._next("snap")
        return self.z["snap_ints"][i].copy(), self.z["snap_dbls"][i].copy(), self.z["snap_rng"][i].copy()

    def finish(self):
        """Every recorded call was asked for: the test ran the whole recorded script."""
        for what, key in (("reset", "reset_seed"), ("mask", "mask"), ("step", "step_args"), ("snap", "snap_ints")):
            assert self.at[what] == len(self.z[key]), \
                f"{self.case}: {self.at[what]} {what} calls made, {len(self.z[key])} recorded"


# set by oracle/gen_golden.py --vs-reference: module -> {case: Recorder}; None = play back
recording: dict | None = None


def reference_env(module: str, case: str, make):
    """The reference env of one test case: played back from the fixture, or (while the fixture is being generated)
    `make()`, the live reference env, wrapped in a Recorder."""
    if recording is None:
        return Playback(module, case)
    rec = Recorder(make())
    recording.setdefault(module, {})[case] = rec
    return rec
