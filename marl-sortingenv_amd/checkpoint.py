"""Checkpoint and resume of a training run, bit for bit (SB3's `model.save` / `load`, src/training.py:199-212, plus the
env state the reference never saves).

`save_checkpoint` composes the `state_dict()`s of the objects that carry run state - `PPOLearner` (weights, Adam's m / v /
step, the shuffle's epoch counter and CPU generator, the position on the schedules, the best evaluation, the episode
carry), the rollout collector with its `BatchedSortingEnv` (`mse_get_state`'s record, the policy stream's step counter)
and any frozen `MlpPolicy` - into ONE `torch.save` file; `load_checkpoint` puts them back into freshly constructed
objects.  The promise is equality, not closeness: 2 iterations, checkpoint, load into fresh objects, 2 more iterations
give the records, weights, optimiser state and env state of 4 iterations run straight through
(tests/test_gpu_checkpoint.py).

A checkpoint holds tensors and plain containers only, so it loads with `torch.load(..., weights_only=True)`; that is
how `load_checkpoint` reads it.  Deliberately NOT in it: schedule callables (construct the learner with them again; strict
loading checks that the same fields are scheduled), the env's `reward` / `done` / `terminal_obs` of the last step (outputs,
not state), and the evaluation env (`evaluate_policy` resets it every time).

This is host work between two updates: a handful of device-to-host copies, no kernel.  The functions of plain data
below (`validate_tree`, `diff_fields` / `check_fingerprint`, `check_format_version`, `format_path`, `atomic_save`,
`generator_state` / `set_generator_state`) need no device.
"""
from __future__ import annotations

import math
import os
import tempfile
from typing import Callable, Mapping, Optional

import torch

FORMAT_VERSION = 1
SECTIONS = ("learner", "collector", "policies")


# ---- plain data: what may be in a checkpoint ------------------------------------------------------------------------------
def validate_tree(tree, where: str = "checkpoint") -> None:
    """Raises TypeError naming the offending path unless `tree` is made of CPU tensors, None, bools, ints, floats,
    strings, lists / tuples and dicts with string or int keys: what `torch.load(weights_only=True)` gives back."""
    if tree is None or isinstance(tree, (bool, int, float, str)):
        return
    if isinstance(tree, torch.Tensor):
        if tree.device.type != "cpu":
            raise TypeError(f"{where}: a checkpoint holds CPU tensors, not one on {tree.device}")
        return
    if isinstance(tree, (list, tuple)) and type(tree) in (list, tuple):
        for i, v in enumerate(tree):
            validate_tree(v, f"{where}[{i}]")
        return
    if type(tree) is dict:
        for k, v in tree.items():
            if not isinstance(k, (str, int)) or isinstance(k, bool):
                raise TypeError(f"{where}: dict keys must be str or int, not {type(k).__name__} ({k!r})")
            validate_tree(v, f"{where}[{k!r}]")
        return
    raise TypeError(f"{where}: {type(tree).__name__} cannot be checkpointed (only tensors, numbers, strings, bools, None, "
                    f"lists and dicts)")


def same_value(a, b) -> bool:
    """Equality of two checkpoint values: tensors by dtype, shape and content, floats with NaN equal to NaN, containers
    element by element; a bool is not an int."""
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        return (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape
                and torch.equal(a, b))
    if isinstance(a, bool) != isinstance(b, bool):
        return False
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        return len(a) == len(b) and all(same_value(x, y) for x, y in zip(a, b))
    if isinstance(a, dict) and isinstance(b, dict):
        return a.keys() == b.keys() and all(same_value(v, b[k]) for k, v in a.items())
    if type(a) is not type(b) and not (isinstance(a, (int, float)) and isinstance(b, (int, float))):
        return False
    return a == b


def _show(v) -> str:
    if isinstance(v, torch.Tensor):
        return f"<{str(v.dtype).replace('torch.', '')}{list(v.shape)}>"
    return repr(v)


def diff_fields(saved: Mapping, mine: Mapping, fields=None) -> list:
    """-> [(field, saved value, own value)] for every field (default: the union of both key sets, sorted) whose values
    differ; a field one side lacks counts as differing and shows as '<absent>'."""
    names = sorted(set(saved) | set(mine), key=str) if fields is None else list(fields)
    absent = "<absent>"
    out = []
    for f in names:
        a, b = saved.get(f, absent), mine.get(f, absent)
        if not same_value(a, b):
            out.append((f, a, b))
    return out


def mismatch_message(what: str, diffs: list) -> str:
    return f"{what} does not match the checkpoint: " + "; ".join(
        f"{f}: checkpoint has {_show(a)}, this object has {_show(b)}" for f, a, b in diffs)


def check_fingerprint(saved: Mapping, mine: Mapping, what: str, fields=None) -> None:
    """ValueError naming every differing field with both values; nothing when there is none."""
    diffs = diff_fields(saved, mine, fields)
    if diffs:
        raise ValueError(mismatch_message(what, diffs))


def check_format_version(version) -> None:
    if isinstance(version, bool) or not isinstance(version, int) or version != FORMAT_VERSION:
        raise ValueError(f"checkpoint format version {version!r} is not one this library reads ({FORMAT_VERSION})")


def format_path(path, iteration: int) -> str:
    """`path` with its `{iteration}` field, if it has one, filled in ("run_{iteration:04d}.pt" keeps every file)."""
    return os.fspath(path).format(iteration=int(iteration))


def atomic_save(tree, path, serializer: Optional[Callable] = None) -> str:
    """Validates `tree`, writes it to a temporary file in `path`'s directory, then `os.replace`s it over `path`.  A
    failure at any point - validation, serialisation, the disk - leaves an earlier file at `path` as it was and removes
    the temporary one.  serializer(tree, file object): `torch.save` unless given."""
    validate_tree(tree)
    path = os.fspath(path)
    fd, tmp = tempfile.mkstemp(prefix=os.path.basename(path) + ".", suffix=".tmp", dir=os.path.dirname(path) or ".")
    try:
        with os.fdopen(fd, "wb") as f:
            (torch.save if serializer is None else serializer)(tree, f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        try:
            os.unlink(tmp)
        except OSError:
            pass
        raise
    return path


def generator_state(generator: torch.Generator) -> torch.Tensor:
    """A CPU generator's state as `get_state()`'s byte tensor (a copy)."""
    return generator.get_state().clone()


def set_generator_state(generator: torch.Generator, state: torch.Tensor) -> None:
    generator.set_state(state.to(device="cpu", dtype=torch.uint8).contiguous())


def cpu(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """A CPU copy that shares nothing with `t` (one blocking device-to-host copy for a device tensor)."""
    return None if t is None else t.detach().to("cpu", copy=True).contiguous()


def check_tensor(sd: Mapping, key: str, like: torch.Tensor, what: str) -> None:
    """ValueError unless sd[key] is a tensor of `like`'s dtype and shape."""
    t = sd.get(key)
    if not isinstance(t, torch.Tensor) or t.dtype != like.dtype or tuple(t.shape) != tuple(like.shape):
        got = _show(t) if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{what}: {key} must be {_show(like)}, the checkpoint has {got}")


# ---- frozen policies ---------------------------------------------------------------------------------------------------------
def policy_state(policy) -> dict:
    """A frozen `MlpPolicy` as its dims and its flat f32 weights (SB3_KEYS order)."""
    return {"obs_dim": policy.obs_dim, "n_actions": policy.n_actions,
            "weights": torch.from_numpy(policy.flat_weights().copy())}


def check_policy_state(sd: Mapping, policy, name: str) -> None:
    check_fingerprint({k: sd.get(k) for k in ("obs_dim", "n_actions")},
                      {"obs_dim": policy.obs_dim, "n_actions": policy.n_actions}, f"policy {name!r}")
    n = int(policy.L.mse_policy_num_weights(policy.obs_dim, policy.n_actions))
    check_tensor(sd, "weights", torch.empty(n, dtype=torch.float32), f"policy {name!r}")


# ---- the file ---------------------------------------------------------------------------------------------------------------
def save_checkpoint(path, learner=None, collector=None, policies: Optional[Mapping] = None, iteration: int = 0,
                    iterations: Optional[int] = None, history: Optional[list] = None, extra=None, envs: bool = True) -> str:
    """Writes one `torch.save` file: the format version, the library's `mse_version()`, `iteration` (the number of
    iterations done), `iterations`, `history` (their records), `extra` (anything of plain data) and the sections
    "learner" (`PPOLearner.state_dict()`), "collector" (`FusedPolicyRollout` / `PolicyRolloutCollector.state_dict()`, which
    holds the env's) and "policies" (name -> `MlpPolicy`: frozen agents such as Env_2's `sort_policy`, as flat weights and
    dims, so a staged sort -> press run restarts from one file).  A section whose object is not given is not written.
    envs=False leaves the collector section out (the env state is 840 B per env): a run resumed from such a file starts
    from reset envs and a policy stream at step 0, so it is a continuation of the weights and the optimiser, not the same
    run.  The eval env needs no state: `evaluate_policy` resets it every time.
    The write is atomic (`atomic_save`); returns the path."""
    from ._lib import load_library

    tree = {"format_version": FORMAT_VERSION, "mse_version": int(load_library().mse_version()),
            "iteration": int(iteration), "iterations": None if iterations is None else int(iterations),
            "history": [dict(r) for r in history] if history is not None else [], "extra": extra}
    if learner is not None:
        tree["learner"] = learner.state_dict()
    if collector is not None and envs:
        tree["collector"] = collector.state_dict()
    if policies:
        tree["policies"] = {str(name): policy_state(p) for name, p in policies.items()}
    return atomic_save(tree, path)


def read_checkpoint(path) -> dict:
    """The file's tree (`torch.load(map_location="cpu", weights_only=True)`) after the format version check."""
    tree = torch.load(os.fspath(path), map_location="cpu", weights_only=True)
    if not isinstance(tree, dict):
        raise ValueError(f"{path} is not a checkpoint of this library")
    check_format_version(tree.get("format_version"))
    return tree


def missing_sections(tree: Mapping, learner=None, collector=None, policies: Optional[Mapping] = None) -> list:
    """The sections (and "policies[name]" entries) that are asked for and not in `tree`."""
    out = [s for s, obj in (("learner", learner), ("collector", collector)) if obj is not None and s not in tree]
    for name in (policies or {}):
        if str(name) not in tree.get("policies", {}):
            out.append(f"policies[{str(name)!r}]")
    return out


def load_checkpoint(path, learner=None, collector=None, policies: Optional[Mapping] = None, strict: bool = True) -> dict:
    """Loads the sections of `path` into the objects given (`load_state_dict` of each; `policies`: name -> `MlpPolicy`,
    loaded with `load_weights`) and returns the rest: {"iteration", "iterations", "history", "extra", "format_version",
    "mse_version" (the writer's), "library_mse_version" (this library's), "loaded" (the sections that were loaded)}.
    Refuses (ValueError) an unknown format version; a section that is asked for and absent - a collector for a file
    written with envs=False, say - unless strict=False, which skips it; and whatever the objects' own `load_state_dict`
    refuse (`strict` is passed on to the learner).  Every check of every object runs before the first byte is copied, so
    a refusal leaves all of them as they were."""
    from ._lib import load_library

    tree = read_checkpoint(path)
    missing = missing_sections(tree, learner, collector, policies)
    if missing and strict:
        raise ValueError(f"the checkpoint {os.fspath(path)} has no " + ", ".join(missing)
                         + " (strict=False loads what is there)")
    todo = []
    if collector is not None and "collector" in tree:
        collector.check_state_dict(tree["collector"])
        todo.append(("collector", lambda: collector.load_state_dict(tree["collector"])))
    for name, pol in (policies or {}).items():
        sd = tree.get("policies", {}).get(str(name))
        if sd is not None:
            check_policy_state(sd, pol, str(name))
            todo.append((f"policies[{str(name)!r}]", lambda pol=pol, sd=sd: pol.load_weights(sd["weights"])))
    if learner is not None and "learner" in tree:
        learner.check_state_dict(tree["learner"], strict=strict)
        todo.append(("learner", lambda: learner.load_state_dict(tree["learner"], strict=strict)))
    for _, apply in todo:
        apply()
    return {"iteration": tree.get("iteration", 0), "iterations": tree.get("iterations"), "history": tree.get("history", []),
            "extra": tree.get("extra"), "format_version": tree["format_version"], "mse_version": tree.get("mse_version"),
            "library_mse_version": int(load_library().mse_version()), "loaded": [name for name, _ in todo]}
