"""GPU: the learner's device permutation.  `k_ppo_shuffle` (mse_ppo_shuffle) against its host twin
(mse_ppo_shuffle_host, which tests/test_ppo_shuffle_cpu.py holds against an independent restatement) bit for bit, at
every store path of the kernel: 16-byte pairs, the 8-byte head of an output that is not 16-byte aligned, the odd tail,
windows of one to three rows, the grid-stride loop past the grid cap, a non-default stream; and
`PPOLearner(shuffle="device").update()` against an update written out by hand from `permutation()`, `loss_grad` and
`adam_step`, bit for bit (the gradient path has no atomics: equal rows give equal bits)."""
import ctypes as C

import numpy as np
import pytest

from tests.ppo_checks import DIMS, HP, make_policy

pytestmark = pytest.mark.gpu

SEED, EPOCH = 2 ** 40 + 5, 3
BAND, SENTINEL = 64, -7
ROWS_PER_GROUP, GROUPS_PER_CU = 512, 8  # k_ppo_shuffle: 256 lanes x 2 rows per trip; at most 8 workgroups per CU


def _host(total, seed=SEED, epoch=EPOCH):
    import torch

    import marl_sortingenv_amd as M

    rows = torch.empty(total, dtype=torch.int64)
    assert M.load_library().mse_ppo_shuffle_host(total, seed, epoch, 0, total, C.c_void_p(rows.data_ptr())) == 0
    return rows


def _device_window(total, first, count, misaligned, seed=SEED, epoch=EPOCH):
    """mse_ppo_shuffle into a sentinel-filled buffer between guard bands, at an output address that is a multiple of
    16 bytes or (misaligned) 8 past one; returns the window after checking that nothing else was written."""
    import torch

    import marl_sortingenv_amd as M

    lead = BAND + (1 if misaligned else 0)
    buf = torch.full((lead + count + BAND,), SENTINEL, dtype=torch.int64, device="cuda")
    out = buf[lead:lead + count]
    assert buf.data_ptr() % 16 == 0 and (buf.data_ptr() + 8 * lead) % 16 == (8 if misaligned else 0)
    stream = torch.cuda.current_stream()
    rc = M.load_library().mse_ppo_shuffle(total, seed, epoch, first, count, C.c_void_p(buf.data_ptr() + 8 * lead),
                                          C.c_void_p(stream.cuda_stream))
    assert rc == 0, M.load_library().mse_last_error()
    stream.synchronize()
    assert bool((buf[:lead] == SENTINEL).all()) and bool((buf[lead + count:] == SENTINEL).all()), (total, first, count)
    return out.cpu()


def _windows(total):
    """(first, count): the whole range, odd starts, counts of 1, 2 and 3 at the front, at odd starts and ending at total - 1"""
    w = {(0, total), (0, 0), (total, 0)}
    for count in (1, 2, 3):
        for first in (0, 1, 3, total - count, total - count - 1):
            if first >= 0 and first + count <= total:
                w.add((first, count))
    for first in (1, 3, 5):
        if first < total:
            w.add((first, total - first))      # odd start, ends at total - 1
            w.add((first, total - first - 1))  # odd start, ends at total - 2
    return sorted(w)


@pytest.mark.parametrize("total", [1, 2, 63, 64, 65, 4097, 65537, 2 ** 20 + 1])
def test_kernel_equals_host_twin(total):
    import torch

    want = _host(total)
    assert torch.equal(want.sort().values, torch.arange(total))
    for first, count in _windows(total):
        for misaligned in (False, True):
            got = _device_window(total, first, count, misaligned)
            assert np.array_equal(got.numpy(), want[first:first + count].numpy()), (total, first, count, misaligned)


def _grid_cap():
    import torch

    return GROUPS_PER_CU * torch.cuda.get_device_properties(0).multi_processor_count  # workgroups of k_ppo_shuffle at most


def test_grid_stride_loop_past_the_grid_cap():
    """cap x 512 rows fill every lane's first trip; five more give two lanes a second pair and leave an odd row"""
    total = _grid_cap() * ROWS_PER_GROUP + 5
    want = _host(total, seed=9, epoch=2 ** 33)
    for first, misaligned in ((0, False), (0, True), (1, False)):
        got = _device_window(total, first, total - first, misaligned, seed=9, epoch=2 ** 33)
        assert np.array_equal(got.numpy(), want[first:].numpy()), (total, first, misaligned)


def test_non_default_stream():
    import torch

    total = 65537
    want = _host(total)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream() == side
        got = _device_window(total, 1, total - 1, True)
    assert np.array_equal(got.numpy(), want[1:].numpy())


def test_device_call_refuses_what_the_host_call_refuses():
    import torch

    import marl_sortingenv_amd as M

    L = M.load_library()
    buf = torch.full((16,), SENTINEL, dtype=torch.int64, device="cuda")
    p, s = C.c_void_p(buf.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for total, first, count, ptr in ((0, 0, 0, p), (2 ** 31 + 1, 0, 1, p), (100, -1, 1, p), (100, 0, -1, p), (100, 99, 2, p),
                                     (100, 101, 0, p), (100, 0, 4, None)):
        assert L.mse_ppo_shuffle(total, 5, 3, first, count, ptr, s) == -1, (total, first, count)
    assert L.mse_ppo_shuffle(100, 5, 3, 50, 0, None, s) == 0
    torch.cuda.synchronize()
    assert buf.tolist() == [SENTINEL] * 16


# ---- the learner -----------------------------------------------------------------------------------------------------------
CFG = dict(n=300, K=16, n_epochs=3, learning_rate=1e-3)


def _setup(kind, batch_size, seed=5, shuffle="device"):
    import marl_sortingenv_amd as M

    pol, flat = make_policy(*DIMS[kind], 31, precision="f32")
    env = M.BatchedSortingEnv(kind=kind, num_envs=CFG["n"], device=0, base_seed=21, max_steps=5, noise_sorting=0.05, balesize=200,
                              auto_reset=True)
    col = M.FusedPolicyRollout(env, pol, CFG["K"], seed=22)
    learner = M.PPOLearner(pol, learning_rate=CFG["learning_rate"], n_epochs=CFG["n_epochs"], batch_size=batch_size, seed=seed,
                           shuffle=shuffle, **HP)
    return pol, col, learner


def _update_by_hand(hand, data, epochs, bs):
    """What update() is specified to do, from the public pieces: rows of `permutation(total, epoch)`, loss_grad, adam_step."""
    import torch

    import marl_sortingenv_amd as M

    M.compute_gae(data, hand.gamma, hand.gae_lambda)
    total = data["rewards"].numel()
    stats = torch.zeros((len(epochs) * -(-total // bs), 8), device="cuda")
    i = 0
    for epoch in epochs:
        rows = hand.permutation(total, epoch)
        assert rows.device.type == "cpu" and rows.dtype == torch.int64 and sorted(rows.tolist()) == list(range(total))
        rows = rows.cuda()
        for start in range(0, total, bs):
            mb = rows[start:start + bs]
            hand.loss_grad(data, mb, mb.numel(), stats[i])
            hand.adam_step()
            i += 1
    return stats


def _same_bits(a, b):
    import torch

    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# default batch (4 800 / 4 = 1 200 rows), a short last minibatch (4 x 1 000 + 800), another env shape
@pytest.mark.parametrize("kind,batch_size", [("mono", None), ("mono", 1000), ("press", None)])
def test_update_equals_an_update_written_out_by_hand(kind, batch_size, monkeypatch):
    import torch

    pol, col, learner = _setup(kind, batch_size)
    _, _, hand = _setup(kind, batch_size, shuffle="cpu")  # its own policy and Adam state; only the public pieces are used
    total = CFG["n"] * CFG["K"]
    bs = batch_size if batch_size is not None else (total + 3) // 4
    per_epoch = -(-total // bs)
    assert (total % bs != 0) == (batch_size == 1000)
    n_updates = 2 if (kind, batch_size) == ("mono", None) else 1

    def no_randperm(*a, **k):
        raise AssertionError("shuffle='device' must not call torch.randperm")

    for u in range(n_updates):
        data = col.collect()
        with monkeypatch.context() as mp:
            mp.setattr(torch, "randperm", no_randperm)
            out = learner.update(data)
        torch.cuda.synchronize()
        epochs = list(range(u * CFG["n_epochs"], (u + 1) * CFG["n_epochs"]))
        assert learner.last_epochs == epochs and learner.epochs_done == epochs[-1] + 1 and learner.last_permutations == []
        assert out["stats"].shape == (CFG["n_epochs"] * per_epoch, 8) and learner.step == (u + 1) * CFG["n_epochs"] * per_epoch
        want_stats = _update_by_hand(hand, data, epochs, bs)
        torch.cuda.synchronize()
        for name in ("weights", "m", "v"):
            assert _same_bits(getattr(learner, name), getattr(hand, name)), (kind, batch_size, u, name)
        assert _same_bits(out["stats"], want_stats), (kind, batch_size, u)
        assert np.array_equal(pol.flat_weights(), learner.weights.cpu().numpy())  # the rollout policy got the new weights
        # the buffer holds the last epoch's permutation and is reused while the rollout size stays
        assert torch.equal(learner._perm.cpu(), learner.permutation(total, epochs[-1]))
        if u == 0:
            ptr = learner._perm.data_ptr()
        assert learner._perm.data_ptr() == ptr
    assert not torch.equal(learner.permutation(total, 0), learner.permutation(total, 1))


def test_same_seed_same_weights_other_seed_other_weights():
    def run(seed):
        pol, col, learner = _setup("mono", 1000, seed=seed)
        history = learner.learn(col, iterations=2)
        assert len(history) == 2 and learner.last_epochs == [3, 4, 5] and learner.last_permutations == []
        return learner.weights.cpu()

    a, b, c = run(5), run(5), run(5 + 2 ** 32)
    assert _same_bits(a, b)
    assert not _same_bits(a, c)


def test_cpu_mode_is_the_default_and_keeps_its_record():
    import torch

    pol, col, learner = _setup("mono", None, shuffle="cpu")
    assert learner.shuffle == "cpu"
    learner.update(col.collect())
    torch.cuda.synchronize()
    g = torch.Generator().manual_seed(5)
    assert len(learner.last_permutations) == CFG["n_epochs"] and learner.last_epochs == [] and learner.epochs_done == 0
    for p in learner.last_permutations:
        assert torch.equal(p, torch.randperm(CFG["n"] * CFG["K"], generator=g))


def test_unknown_shuffle_is_refused():
    import marl_sortingenv_amd as M

    pol, _ = make_policy(*DIMS["mono"], 31)
    with pytest.raises(ValueError):
        M.PPOLearner(pol, shuffle="nonsense")
    assert M.PPOLearner(pol).shuffle == "cpu"
