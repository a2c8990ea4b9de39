"""Device forward of the reference's actor-critic policy.

The reference trains `MaskablePPO(MaskableActorCriticPolicy, net_arch=dict(pi=[32, 32], vf=[32, 32]))`
(src/training.py:115-131): two separate 2x32 tanh MLPs, a linear action head and a linear value head; invalid
actions get logit -1e8 before the softmax.  `MlpPolicy.forward` evaluates that network for a whole batch of
observations on the f32 matrix cores (`mse_policy_forward`, csrc/mse_policy.hip) and samples actions with the
engine's counter-based stream, so `env.step(policy.forward(obs, mask)["action"])` never leaves the device.
PyTorch is plumbing here (device memory, stream); no torch op computes anything on this path.
"""
from __future__ import annotations

import ctypes as C
from typing import Mapping, Optional

import numpy as np
import torch

from ._lib import check, load_library

HIDDEN = 32
# torch.nn.Linear tensors in the order include/mse.h documents, under the names SB3's state_dict gives them
SB3_KEYS = [
    "mlp_extractor.policy_net.0.weight", "mlp_extractor.policy_net.0.bias",
    "mlp_extractor.policy_net.2.weight", "mlp_extractor.policy_net.2.bias",
    "action_net.weight", "action_net.bias",
    "mlp_extractor.value_net.0.weight", "mlp_extractor.value_net.0.bias",
    "mlp_extractor.value_net.2.weight", "mlp_extractor.value_net.2.bias",
    "value_net.weight", "value_net.bias",
]


def _shapes(obs_dim: int, n_actions: int):
    H = HIDDEN
    return [(H, obs_dim), (H,), (H, H), (H,), (n_actions, H), (n_actions,),
            (H, obs_dim), (H,), (H, H), (H,), (1, H), (1,)]


class MlpPolicy:
    """weights: mapping from the SB3 state_dict names (SB3_KEYS) to arrays / tensors of the documented shapes."""

    PRECISIONS = {"auto": 0, "f32": 1, "f16x3": 2}

    def __init__(self, obs_dim: int, n_actions: int, weights: Mapping[str, object], device: int | str | torch.device = 0,
                 library: Optional[str] = None, precision: str = "auto"):
        if not torch.cuda.is_available():
            raise RuntimeError("MlpPolicy needs a HIP device: there is no CPU fallback")
        self.L = load_library(library)
        self.obs_dim, self.n_actions = int(obs_dim), int(n_actions)
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        parts = []
        for key, shape in zip(SB3_KEYS, _shapes(self.obs_dim, self.n_actions)):
            if key not in weights:
                raise KeyError(f"missing weight {key!r}")
            w = weights[key]
            w = w.detach().cpu().numpy() if isinstance(w, torch.Tensor) else np.asarray(w)
            if tuple(w.shape) != tuple(shape):
                raise ValueError(f"{key}: shape {tuple(w.shape)}, expected {tuple(shape)}")
            parts.append(np.ascontiguousarray(w, dtype=np.float32).ravel())
        blob = np.concatenate(parts)
        assert blob.size == self.L.mse_policy_num_weights(self.obs_dim, self.n_actions)
        self.weights = {k: p.copy() for k, p in zip(SB3_KEYS, parts)}
        h = C.c_void_p()
        dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        check(self.L.mse_policy_create(C.byref(h), self.obs_dim, self.n_actions,
                                       blob.ctypes.data_as(C.POINTER(C.c_float)), dev_index))
        self._h = h
        self.set_precision(precision)

    @property
    def weights(self) -> dict:
        """The weights under SB3_KEYS as flat numpy arrays.  After `load_weights_device` the first access reads them back
        from the handle's own device copy (`mse_policy_get_weights`, a blocking copy)."""
        if self._weights is None:
            flat = np.empty(self.L.mse_policy_num_weights(self.obs_dim, self.n_actions), dtype=np.float32)
            with torch.cuda.device(self.device):
                check(self.L.mse_policy_get_weights(self._h, C.c_void_p(flat.ctypes.data)))
            sizes = [int(np.prod(s)) for s in _shapes(self.obs_dim, self.n_actions)]
            self._weights = dict(zip(SB3_KEYS, np.split(flat, np.cumsum(sizes)[:-1])))
        return self._weights

    @weights.setter
    def weights(self, value: dict) -> None:
        self._weights = value

    def set_precision(self, precision: str) -> str:
        """"f32": exact f32 matrix products; "f16x3": three f16 MFMAs per product on 22-bit operand splits (logits
        within ~1e-6 of f32 at SB3-scale weights, ~3e-5 of float64 with hidden pre-activations of ~40; 5x the matrix
        rate); "auto": f16x3 when the weights fit f16's range.  Returns the form in effect."""
        check(self.L.mse_policy_set_precision(self._h, self.PRECISIONS[precision]))
        self.precision = "f16x3" if self.L.mse_policy_precision(self._h) == 2 else "f32"
        return self.precision

    @classmethod
    def from_state_dict(cls, state_dict: Mapping[str, object], device=0, library: Optional[str] = None) -> "MlpPolicy":
        """From `model.policy.state_dict()` of the reference's (Maskable)PPO; dimensions are read off the tensors."""
        w1 = state_dict["mlp_extractor.policy_net.0.weight"]
        wa = state_dict["action_net.weight"]
        return cls(int(w1.shape[1]), int(wa.shape[0]), state_dict, device=device, library=library)

    @classmethod
    def random_init(cls, obs_dim: int, n_actions: int, seed: int = 0, device=0, library: Optional[str] = None,
                    precision: str = "auto") -> "MlpPolicy":
        """Random weights of the reference's architecture in SB3's initial scale (orthogonal-like magnitudes: hidden
        layers ~ sqrt(2) / sqrt(fan_in), action head 0.01, value head 1) - for benchmarks and smoke runs."""
        rng = np.random.default_rng(seed)
        w = {}
        for key, shape in zip(SB3_KEYS, _shapes(obs_dim, n_actions)):
            if len(shape) == 1:
                w[key] = np.zeros(shape, dtype=np.float32)
            else:
                gain = 0.01 if key == "action_net.weight" else (1.0 if key == "value_net.weight" else np.sqrt(2.0))
                w[key] = (rng.standard_normal(shape) * gain / np.sqrt(shape[1])).astype(np.float32)
        return cls(obs_dim, n_actions, w, device=device, library=library, precision=precision)

    def load_weights(self, weights) -> "MlpPolicy":
        """Replaces the weights in place (`mse_policy_set_weights`: the same host repacking as at creation, then a
        blocking copy).  `weights`: a mapping under SB3_KEYS, or the flat vector in that order (array / tensor, any
        device).  No rollout or forward on this policy may be in flight on another stream.  Refreshes `self.weights`
        and `self.precision` (an "auto" policy moves to f32 when a folded weight leaves f16's range)."""
        shapes = _shapes(self.obs_dim, self.n_actions)
        if isinstance(weights, Mapping):
            parts = []
            for key, shape in zip(SB3_KEYS, shapes):
                if key not in weights:
                    raise KeyError(f"missing weight {key!r}")
                w = weights[key]
                w = w.detach().cpu().numpy() if isinstance(w, torch.Tensor) else np.asarray(w)
                if tuple(w.shape) != tuple(shape):
                    raise ValueError(f"{key}: shape {tuple(w.shape)}, expected {tuple(shape)}")
                parts.append(np.ascontiguousarray(w, dtype=np.float32).ravel())
            blob = np.concatenate(parts)
        else:
            w = weights.detach().cpu().numpy() if isinstance(weights, torch.Tensor) else np.asarray(weights)
            blob = np.ascontiguousarray(w, dtype=np.float32).ravel()
        n = self.L.mse_policy_num_weights(self.obs_dim, self.n_actions)
        if blob.size != n:
            raise ValueError(f"expected {n} weights, got {blob.size}")
        check(self.L.mse_policy_set_weights(self._h, blob.ctypes.data_as(C.POINTER(C.c_float))))
        sizes = [int(np.prod(s)) for s in shapes]
        self.weights = {k: p.copy() for k, p in zip(SB3_KEYS, np.split(blob, np.cumsum(sizes)[:-1]))}
        self.precision = "f16x3" if self.L.mse_policy_precision(self._h) == 2 else "f32"
        return self

    def load_weights_device(self, weights: torch.Tensor, sync: bool = True) -> "MlpPolicy":
        """Replaces the weights from a flat f32 device tensor (SB3_KEYS order) without the host: one launch on the current
        stream repacks them on the device (`mse_policy_set_weights_device`, the image `load_weights` would write, byte
        for byte) and copies them into a buffer the handle owns, which `weights`, `flat_weights()` and `state_dict()`
        read back on their next use - `weights` itself may be overwritten afterwards.  Launches enqueued on that stream
        afterwards see the new weights; for other streams the rule of `load_weights` stands.
        sync=True: `sync()` right away.  sync=False: nothing waits; call `sync()` before the next launch whenever the new
        weights may cross f16's range - until then `precision` and the launches keep the form last known."""
        n = self.L.mse_policy_num_weights(self.obs_dim, self.n_actions)
        if not isinstance(weights, torch.Tensor) or weights.device != self.device or weights.dtype != torch.float32 \
                or not weights.is_contiguous():
            raise ValueError(f"weights must be a contiguous float32 tensor on {self.device}")
        if weights.numel() != n:
            raise ValueError(f"expected {n} weights, got {weights.numel()}")
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            check(self.L.mse_policy_set_weights_device(self._h, C.c_void_p(weights.data_ptr()), stream))
        self._weights = None  # read back from the handle on the next access
        if sync:
            self.sync()
        return self

    def sync(self) -> str:
        """After `load_weights_device(sync=False)`: one small blocking read (`mse_policy_sync`) that brings `precision`
        up to date (an "auto" policy moves to f32 when a folded weight has left f16's range, and back).  Raises MseError
        when the policy is pinned to f16x3 and refused the weights: it then still holds the previous ones."""
        with torch.cuda.device(self.device):
            check(self.L.mse_policy_sync(self._h))
        self.precision = "f16x3" if self.L.mse_policy_precision(self._h) == 2 else "f32"
        return self.precision

    def flat_weights(self) -> np.ndarray:
        """The weights as one float32 vector in the order of include/mse.h (SB3_KEYS)."""
        return np.concatenate([self.weights[k].ravel() for k in SB3_KEYS])

    def state_dict(self) -> dict:
        """CPU torch tensors under SB3's state_dict names and shapes: `torch.save` it, or load it into the
        `mlp_extractor` / `action_net` / `value_net` of an SB3 (Maskable)ActorCriticPolicy elsewhere."""
        return {k: torch.from_numpy(self.weights[k].reshape(s).copy())
                for k, s in zip(SB3_KEYS, _shapes(self.obs_dim, self.n_actions))}

    def close(self):
        if getattr(self, "_h", None):
            self.L.mse_policy_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def forward(self, obs: torch.Tensor, mask: Optional[torch.Tensor] = None, seed: int = 2024, t: int = 0,
                deterministic: bool = False, index_offset: int = 0, want_logits: bool = False,
                out: Optional[dict] = None) -> dict:
        """obs f32[N, D] (device), mask u8/bool[N, A] or None -> {"action" i32[N], "logp" f32[N], "value" f32[N]
        [, "logits" f32[N, A]]}."""
        if obs.dim() != 2 or obs.shape[1] != self.obs_dim:
            raise ValueError(f"obs must be [N, {self.obs_dim}]")
        obs = obs.to(device=self.device, dtype=torch.float32).contiguous()
        n = obs.shape[0]
        if mask is not None:
            if tuple(mask.shape) != (n, self.n_actions):
                raise ValueError(f"mask must be [N, {self.n_actions}]")
            mask = mask.to(device=self.device, dtype=torch.uint8).contiguous()
        if out is None:  # pass a previous result back in to reuse its buffers
            out = {
                "action": torch.empty((n,), dtype=torch.int32, device=self.device),
                "logp": torch.empty((n,), dtype=torch.float32, device=self.device),
                "value": torch.empty((n,), dtype=torch.float32, device=self.device),
            }
            if want_logits:
                out["logits"] = torch.empty((n, self.n_actions), dtype=torch.float32, device=self.device)

        def ptr(x):
            return None if x is None else C.c_void_p(x.data_ptr())

        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            check(self.L.mse_policy_forward(self._h, n, int(index_offset), ptr(obs), ptr(mask), int(seed), int(t),
                                            1 if deterministic else 0, ptr(out["action"]), ptr(out["logp"]),
                                            ptr(out["value"]), ptr(out.get("logits")), stream))
        return out
