"""The one-pass L1 kernels (ibgs_amd/csrc/loss.hip) on every path: the float4 body with its scalar tail and the pure scalar loop that any pointer off
16-byte alignment selects, sizes below one quad, around the 4096-element block quantum, past the 1024-block cap of `l1_partial_kernel` and past the
4096-block cap of `l1_grad_kernel` / `l1_rescale_kernel` (a second trip of the grid-stride loop) -- through the C ABI and through `losses.l1_loss`.

Value: against `exact` = the float64 sum of |fp32(a - b)| over n (numpy, host).  A thread adds at most m = max(16, ceil(n / 262144)) + 5 terms in fp32
(4 quads of 4 up to the block cap, n / (1024 * 256) beyond it, one tail element, slack) before the sums go on in double, and the result is rounded to
fp32 once: |got - exact| <= m * 2^-24 * exact.  From the accumulation scheme, not measured.

Gradient: one of 0, +-fl32(1 / n) with the division in double; after a backward with the fp32 scalar w, +-fl32(fl32(1 / n) * w).  Restated in numpy and
compared as integers (a zero is a zero whatever its sign bit)."""
import math

import numpy as np
import pytest
import torch

from ibgs_amd import _lib
from ibgs_amd.losses import l1_loss

pytestmark = pytest.mark.gpu
DEV = "cuda"
WEIGHTS = (1.0, 0.75, -2.0, 0.0)
SMALL = (1, 2, 3, 4, 5, 4095, 4096, 4097)
PAST_PARTIAL_CAP = 1024 * 4096 + 4097
PAST_GRAD_CAP = 4096 * 4096 + 5


def _pair(n, seed):
    """a, b on the host (fp32 numpy): noise, exact ties, differences that are denormal, zeros of both signs."""
    rng = np.random.default_rng(seed)
    a, b = rng.random(n, dtype=np.float32), rng.random(n, dtype=np.float32)
    a[6::7] = b[6::7]                                     # ties: sign(0) = 0
    special = [(1.5e-38, 1.4e-38), (1.4e-38, 1.5e-38), (0.0, -0.0), (-0.0, 0.0), (-0.0, -0.0), (1.0, 1.0 - 2.0 ** -24), (2e-45, 0.0), (0.0, 1e-45)]
    for k, (p, q) in enumerate(special):
        i = 3 * k + 2                                     # (from the third element on: the value of n = 1, 2 stays in the normal range, where the bound below holds)
        if i < n:
            a[i], b[i] = p, q
    return a, b


def _unit_bits(a, b, w=None):
    """The restated gradient as int32 bit patterns, zeros normalised to +0."""
    n = a.size
    d = a - b                                             # fp32, denormals kept
    k = np.float32(1.0 / n)                               # the division in double, rounded once
    if w is not None:
        k = np.float32(k * np.float32(w))
    g = np.where(d > 0, k, np.where(d < 0, -k, np.float32(0.0))).astype(np.float32)
    return _norm_bits(torch.from_numpy(g))


def _norm_bits(t):
    t = t.detach().reshape(-1)
    return torch.where(t == 0, torch.zeros_like(t), t).view(torch.int32)


def _exact(a, b):
    return float(np.abs(a - b).astype(np.float64).sum() / a.size)


def _check_value(got, a, b):
    n, exact = a.size, _exact(a, b)
    m = max(16, math.ceil(n / 262144)) + 5
    err = abs(float(got) - exact)
    print("[l1 edges] n=%d: value %.9g, exact %.9g, |err| %.2e, bound %.2e" % (n, float(got), exact, err, m * 2.0 ** -24 * exact))
    assert err <= m * 2.0 ** -24 * exact


class _Carved:
    """`n` fp32 words at element offset `off` of a larger allocation: offset 1 is 4 bytes off 16-byte alignment."""

    def __init__(self, n, off, data=None):
        self.base = torch.full((n + 8,), float("nan"), device=DEV)
        self.t = self.base[off:off + n]
        if data is not None:
            self.t.copy_(torch.from_numpy(data))
        assert self.t.data_ptr() % 16 == 4 * off

    def ptr(self):
        return self.t.data_ptr()


def _scratch(lib):
    return torch.empty(lib.ibgs_required_l1(), dtype=torch.uint8, device=DEV)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _loss(lib, n, x, y, grad, sc):
    out = torch.full((1,), float("nan"), device=DEV)
    rc = lib.ibgs_l1_loss(_stream(), n, x.ptr(), y.ptr(), None if grad is None else grad.ptr(), out.data_ptr(), sc.data_ptr(), sc.numel())
    assert rc == 0, _lib.last_error()
    return out


def _scalar(w):
    return torch.tensor([w], dtype=torch.float32, device=DEV)


def test_every_alignment_of_x_y_and_grad():
    lib, n = _lib.load(), 4097
    a, b = _pair(n, 1)
    sc = _scratch(lib)
    want_unit, want_w = _unit_bits(a, b).to(DEV), _unit_bits(a, b, 0.75).to(DEV)
    w = _scalar(0.75)
    first = {}
    for ox in (0, 1):
        for oy in (0, 1):
            for og in (0, 1):
                x, y = _Carved(n, ox, a), _Carved(n, oy, b)
                g = _Carved(n, og)
                v = _loss(lib, n, x, y, g, sc)
                _check_value(v.cpu()[0], a, b)
                bits = _norm_bits(g.t)
                assert torch.equal(bits, want_unit), (ox, oy, og)
                assert torch.equal(bits, first.setdefault("loss", bits))                 # = the all-aligned run, bit for bit
                assert torch.isnan(g.base[:og]).all() and torch.isnan(g.base[og + n:]).all()
                g2 = _Carved(n, og)
                assert lib.ibgs_l1_grad(_stream(), n, x.ptr(), y.ptr(), w.data_ptr(), g2.ptr()) == 0
                bits2 = _norm_bits(g2.t)
                assert torch.equal(bits2, want_w), (ox, oy, og)
                assert torch.equal(bits2, first.setdefault("grad", bits2))
                assert torch.isnan(g2.base[:og]).all() and torch.isnan(g2.base[og + n:]).all()
                g3 = _Carved(n, og)
                assert lib.ibgs_l1_grad(_stream(), n, x.ptr(), y.ptr(), None, g3.ptr()) == 0     # no scale: the unit gradient
                assert torch.equal(_norm_bits(g3.t), want_unit), (ox, oy, og)
    for og in (0, 1):
        for wv in WEIGHTS:
            g = _Carved(n, og)
            g.t.copy_(want_unit.view(torch.float32))
            assert lib.ibgs_l1_rescale(_stream(), n, g.ptr(), _scalar(wv).data_ptr()) == 0
            assert torch.equal(_norm_bits(g.t), _unit_bits(a, b, wv).to(DEV)), (og, wv)
            assert torch.isnan(g.base[:og]).all() and torch.isnan(g.base[og + n:]).all()


@pytest.mark.parametrize("n", SMALL + (PAST_PARTIAL_CAP,))
@pytest.mark.parametrize("ox", [0, 1])
def test_sizes_through_the_c_abi(n, ox):
    lib = _lib.load()
    a, b = _pair(n, n)
    sc = _scratch(lib)
    x, y, g = _Carved(n, ox, a), _Carved(n, 0, b), _Carved(n, 0)
    v = _loss(lib, n, x, y, g, sc)
    _check_value(v.cpu()[0], a, b)
    unit = _unit_bits(a, b).to(DEV)
    assert torch.equal(_norm_bits(g.t), unit)
    assert torch.isnan(g.base[n:]).all()
    # value-only call: same bits as with a gradient, every time
    vals = [_loss(lib, n, x, y, None, sc) for _ in range(3)]
    assert all(torch.equal(t.view(torch.int32), v.view(torch.int32)) for t in vals)
    for wv in (0.75, -2.0):
        g2 = _Carved(n, 0)
        assert lib.ibgs_l1_grad(_stream(), n, x.ptr(), y.ptr(), _scalar(wv).data_ptr(), g2.ptr()) == 0
        want = _unit_bits(a, b, wv).to(DEV)
        assert torch.equal(_norm_bits(g2.t), want), wv
        assert lib.ibgs_l1_rescale(_stream(), n, g.ptr(), _scalar(wv).data_ptr()) == 0          # (g: unit, then unit * 0.75, then that * -2)
        if wv == 0.75:
            assert torch.equal(_norm_bits(g.t), want)
    k = np.float32(np.float32(np.float32(1.0 / n) * np.float32(0.75)) * np.float32(-2.0))
    d = a - b
    twice = np.where(d > 0, k, np.where(d < 0, -k, np.float32(0))).astype(np.float32)
    assert torch.equal(_norm_bits(g.t), _norm_bits(torch.from_numpy(twice)).to(DEV))
    assert torch.isnan(g.base[n:]).all() and torch.isnan(g2.base[n:]).all()


@pytest.mark.parametrize("ox", [0, 1])
def test_gradient_kernels_past_their_block_cap(ox):
    """n = 4096 * 4096 + 5: the grid of 4096 blocks covers 16 777 216 elements per trip; the last five (one quad and a tail element, or five scalars) belong to the second."""
    lib, n = _lib.load(), PAST_GRAD_CAP
    a, b = _pair(n, 5)
    x, y, g = _Carved(n, ox, a), _Carved(n, 0, b), _Carved(n, ox)
    assert lib.ibgs_l1_grad(_stream(), n, x.ptr(), y.ptr(), _scalar(0.75).data_ptr(), g.ptr()) == 0
    want = _unit_bits(a, b, 0.75).to(DEV)
    assert torch.equal(_norm_bits(g.t), want)
    assert lib.ibgs_l1_rescale(_stream(), n, g.ptr(), _scalar(-2.0).data_ptr()) == 0
    k = np.float32(np.float32(np.float32(1.0 / n) * np.float32(0.75)) * np.float32(-2.0))
    d = a - b
    twice = np.where(d > 0, k, np.where(d < 0, -k, np.float32(0))).astype(np.float32)
    assert torch.equal(_norm_bits(g.t), _norm_bits(torch.from_numpy(twice)).to(DEV))
    assert torch.isnan(g.base[:ox]).all() and torch.isnan(g.base[ox + n:]).all()


@pytest.mark.parametrize("n", SMALL + (PAST_PARTIAL_CAP,))
@pytest.mark.parametrize("misaligned", [False, True])
def test_the_python_entry_point(n, misaligned):
    """`losses.l1_loss` with the rescale path (first backward) and the recompute path (second backward through the same node), every weight."""
    a, b = _pair(n, n + 1)
    off = 1 if misaligned else 0
    xa, yb = _Carved(n, off, a), _Carved(n, 0, b)
    assert xa.t.is_contiguous()
    for wv in WEIGHTS:
        x = xa.t.detach().requires_grad_(True)
        assert x.data_ptr() % 16 == 4 * off
        loss = l1_loss(x, yb.t)
        if wv == WEIGHTS[0]:
            _check_value(loss.detach().cpu(), a, b)
            with torch.no_grad():
                again = l1_loss(x, yb.t)                   # value only
            assert torch.equal(again.view(torch.int32), loss.detach().view(torch.int32))
        want = _unit_bits(a, b, wv).to(DEV)
        node = loss.grad_fn                                # the loss pass stored the unit gradient on its node ...
        assert node.unit_grad is not None and torch.equal(_norm_bits(node.unit_grad), _unit_bits(a, b).to(DEV))
        (loss * wv).backward(retain_graph=True)            # ... the first backward rescales it in place and hands it on
        assert torch.equal(_norm_bits(x.grad), want), ("rescale", wv)
        assert node.unit_grad is None
        x.grad = None
        (loss * wv).backward()                             # spent: recomputed from x and y
        assert torch.equal(_norm_bits(x.grad), want), ("recompute", wv)
