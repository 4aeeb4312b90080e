"""tests/adam_ref.py, the restatement that the GPU tests of the optimiser compare bits with, checked on the CPU: the float64 form against torch.optim.Adam,
the SH basis against the oracle's eval_sh, and the division by 3K through a 24-bit reciprocal (adam_sh_kernel) as pure integer arithmetic."""
import numpy as np
import pytest
import torch

from tests import adam_ref


def test_float64_restatement_is_torch_adam():
    """Same rule, same operation order: 12 steps agree to an ulp or two (2.2e-16 .. 8.9e-16 absolute on O(1) parameters).  Another formula, such as eps inside
    the bias correction, shows at 1e-8 or more."""
    rng = np.random.default_rng(5)
    shapes, lrs = [(257, 3), (64,)], [1.6e-4, 5e-2]
    params = [torch.nn.Parameter(torch.from_numpy(rng.standard_normal(s))) for s in shapes]
    opt = torch.optim.Adam([{"params": [p], "lr": lr} for p, lr in zip(params, lrs)], lr=0.0, eps=1e-15, foreach=False)
    mine = [[p.detach().numpy().copy(), np.zeros(s), np.zeros(s), 0] for p, s in zip(params, shapes)]
    for it in range(12):
        for j, (p, s) in enumerate(zip(params, shapes)):
            if it == 5 and j == 1:
                p.grad = None          # skipped: its step count does not advance
                continue
            g = rng.standard_normal(s) * 10.0 ** ((it % 5) - 3)
            p.grad = torch.from_numpy(g.copy())
            st = mine[j]
            st[3] += 1
            st[0], st[1], st[2] = adam_ref.adam_step(st[0], g, st[1], st[2], st[3], lrs[j], (0.9, 0.999), 1e-15, np.float64)
        opt.step()
    for p, st in zip(params, mine):
        assert float(opt.state[p]["step"]) == st[3]
        for name, a, b in (("param", p.detach().numpy(), st[0]), ("exp_avg", opt.state[p]["exp_avg"].numpy(), st[1]), ("exp_avg_sq", opt.state[p]["exp_avg_sq"].numpy(), st[2])):
            rel = float(np.max(np.abs(a - b) / np.abs(a)))
            print("[adam host] %s %s: max relative difference %.2e" % (tuple(a.shape), name, rel))
            assert rel <= 1e-13, (name, rel)


def _directions():
    rng = np.random.default_rng(11)
    d = rng.standard_normal((200, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
    diag = np.array([[1, 1, 0], [0, 1, -1], [1, 0, 1], [1, 1, 1], [-1, 1, -1]], np.float64)
    diag /= np.linalg.norm(diag, axis=1, keepdims=True)
    return np.concatenate([d, axes, diag])


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_basis_is_the_oracles_eval_sh(degree):
    """A one-hot coefficient makes eval_sh return that basis function (oracle.eval_sh stops before the 0.5 that the reference adds to every colour)."""
    import oracle
    dirs = _directions()
    N, nb = dirs.shape[0], (degree + 1) ** 2
    B = adam_ref.sh_basis(degree, dirs, np.float64)
    assert B.shape == (N, nb)
    for M in sorted({nb, 16}):
        for k in range(M):
            shs = np.zeros((N, M, 3), np.float32)
            shs[:, k, :] = 1.0
            got = np.asarray(oracle.eval_sh(degree, shs, dirs.astype(np.float32)), np.float64)
            want = np.repeat((B[:, k] if k < nb else np.zeros(N))[:, None], 3, axis=1)          # coefficients above the active degree do not contribute
            if k >= nb:
                assert np.all(got == 0.0), (degree, M, k)
                continue
            err = np.abs(got - want).max() / np.abs(want).max()          # relative to the basis function's size: the oracle is fp32, and the polynomials cancel
            assert err <= 1e-6, (degree, M, k, float(err))


def test_float32_basis_is_the_float64_basis_rounded():
    dirs = _directions()
    a, b = adam_ref.sh_basis(3, dirs, np.float32), adam_ref.sh_basis(3, dirs, np.float64)
    assert a.dtype == np.float32 and np.abs(a - b).max() <= 2e-6          # <= ~8 roundings of 6e-8 on values below 3


def test_sh_grad_restatement_sums_views_and_zeroes_inactive_coefficients():
    rng = np.random.default_rng(2)
    means, cams, dc = rng.standard_normal((9, 3)), rng.standard_normal((3, 3)) * 4, rng.standard_normal((3, 9, 3))
    g = adam_ref.sh_grad_from_views(means, cams, dc, 1, 9)
    assert g.shape == (9, 9, 3) and np.all(g[:, 4:] == 0)
    one = sum(adam_ref.sh_grad_from_views(means, cams[v:v + 1], dc[v:v + 1], 1, 9) for v in range(3))
    assert np.allclose(g, one, rtol=1e-14, atol=0)
    d = means[4] - cams[2]
    d /= np.linalg.norm(d)
    assert np.allclose(adam_ref.sh_grad_from_views(means, cams[2:], dc[2:], 1, 4)[4, 1], -adam_ref.C1 * d[1] * dc[2, 4], rtol=1e-14)


def test_division_by_3k_through_the_24_bit_reciprocal():
    """adam_sh_kernel finds the row of element e of a 64-row slab as (e * ceil(2^24 / 3K)) >> 24, in 32-bit unsigned arithmetic."""
    for K in range(1, 17):
        K3 = 3 * K
        inv = ((1 << 24) + K3 - 1) // K3
        e = np.arange(64 * K3, dtype=np.uint64)
        assert int((e * np.uint64(inv)).max()) < 2 ** 32, K          # the product fits the kernel's uint32_t
        assert np.array_equal((e * np.uint64(inv)) >> np.uint64(24), e // np.uint64(K3)), K
        # (the rounded-down reciprocal is wrong from the first row boundary on: this is what the ceil is for)
        assert not np.array_equal((e * np.uint64((1 << 24) // K3)) >> np.uint64(24), e // np.uint64(K3)), K
