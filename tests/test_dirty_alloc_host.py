"""The dirty-allocation harness (tests/dirty_alloc.py) on the CPU, on toy ops written in torch: a correct op passes under all three fills, each planted
defect is reported, the maximum against an unwritten word passes under 0xFF and is caught only by 0x40 (the reason for the second fill), and
`torch.empty` / `torch.empty_like` are the originals again afterwards.  The last test reads the wrappers' source: they allocate through the two spellings the
harness replaces and through no other, so a later change cannot step around it unnoticed."""
import io
import os
import re
import tokenize

import pytest
import torch

from tests import dirty_alloc as da

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WRAPPERS = ("hourglass.py", "coloragg.py", "losses.py", "image_eval.py", "activations.py", "depthnormal.py", "_device.py")
CPU = torch.device("cpu")
X = torch.rand(3, 5, 7, generator=torch.Generator().manual_seed(1)) + 0.25          # positive: a maximum with 0 is the data's


# ---- toy ops: an output and a scratch arena from torch.empty, as the wrappers take them ---------------------------------------------------------------------
def op_correct(x):
    out = torch.empty(tuple(x.shape), dtype=x.dtype, device=x.device)
    sc = torch.empty(16, dtype=torch.float64, device=x.device)
    sc.zero_()
    sc[:3] += x.double().sum((1, 2))
    out.copy_(2 * x + sc[:3].float().view(3, 1, 1))
    top = torch.empty((), dtype=torch.float32, device=x.device)
    top.copy_(x.max())
    return out, top


def op_skips_the_last_element(x):
    out = torch.empty_like(x)
    out.view(-1)[:-1] = (2 * x).view(-1)[:-1]
    return out


def op_adds_into_uncleared_scratch(x):
    sc = torch.empty(4, dtype=torch.float32, device=x.device)
    sc += x.sum()
    out = torch.empty_like(x)
    out.copy_(x + sc[0])
    return out


def op_max_against_an_unwritten_word(x):
    """fmax as the kernels' fmaxf: a NaN operand gives the other operand."""
    n = x.numel()
    sc = torch.empty(n + 1, dtype=torch.float32, device=x.device)
    sc[:n] = x.reshape(-1)
    out = torch.empty((), dtype=torch.float32, device=x.device)
    out.copy_(torch.fmax(sc[:n].max(), sc[n]))
    return out


def op_writes_one_element_past_its_payload(x):
    """(only where the storage goes on behind the payload, as device memory does behind an allocation: a plain CPU tensor's storage ends with it)"""
    out = torch.empty(x.numel(), dtype=torch.float32, device=x.device)
    out.copy_(x.reshape(-1))
    if out.untyped_storage().nbytes() >= (out.storage_offset() + x.numel() + 1) * 4:
        out.as_strided((x.numel() + 1,), (1,))[x.numel()] = 7.0
    return out


def _under(fill, op):
    with da.dirty(fill, CPU) as d:
        out = op(X)
    return out, d


# ---- the context manager ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", da.FILLS)
def test_blocks_alignment_and_what_is_intercepted(fill):
    real = (torch.empty, torch.empty_like)
    with da.dirty(fill, CPU) as d:
        assert torch.empty is not real[0] and torch.empty_like is not real[1]
        a = torch.empty((3, 5), dtype=torch.float32, device="cpu")
        b = torch.empty(7, dtype=torch.float16, device=CPU)
        c = torch.empty(2, 3, dtype=torch.float64, device="cpu")
        e = torch.empty([4], dtype=torch.int32, device="cpu")
        s = torch.empty((), dtype=torch.float32, device="cpu")
        like = torch.empty_like(a)
        z = torch.empty((0, 3), dtype=torch.float32, device="cpu")
        assert d.count == 7
        # not intercepted: another keyword, no device, another device type, empty_like with a keyword or of a tensor that is not contiguous
        torch.empty((3,), dtype=torch.float32, device="cpu", requires_grad=True)
        torch.empty((3,), dtype=torch.float32)
        torch.empty((3,), dtype=torch.float32, device="meta")
        torch.empty_like(a, dtype=torch.float64)
        torch.empty_like(a.t())
        assert d.count == 7
        for t, shape, dtype in ((a, (3, 5), torch.float32), (b, (7,), torch.float16), (c, (2, 3), torch.float64), (e, (4,), torch.int32), (s, (), torch.float32),
                                (like, (3, 5), torch.float32), (z, (0, 3), torch.float32)):
            assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous() and not t.requires_grad
            assert t.storage_offset() * t.element_size() == da.GUARD
        assert all(bool((d.payload_bytes(i) == fill).all()) for i in range(d.count))
        assert d.payload_bytes(0).numel() == 60 and d.payload_bytes(1).numel() == 14 and d.payload_bytes(4).numel() == 4 and d.payload_bytes(6).numel() == 0
        assert all(raw.numel() == 2 * da.GUARD + (n + 255) // 256 * 256 for raw, n, _, _ in d.blocks)
        want = {0x00: (0.0, 0.0, 0.0, 0), 0x40: (3.00392150878906250, 2.125, 32.50196078431372, 1077952576)}
        if fill in want:
            assert (float(a[0, 0]), float(b[0]), int(e[0])) == want[fill][:2] + want[fill][3:] and abs(float(c[0, 0]) - want[fill][2]) < 1e-12
        else:
            assert bool(torch.isnan(a).all()) and bool(torch.isnan(b).all()) and bool(torch.isnan(c).all())
        a.fill_(1.0)
        b.fill_(1.0)
        s.fill_(1.0)
        assert d.guards_intact() and d.touched() == []
        assert bool((d.payload_bytes(0).view(torch.float32) == 1.0).all())
    assert (torch.empty, torch.empty_like) == real
    assert da.GUARD % 256 == 0 and da.FILLS == (0x00, 0xFF, 0x40)


def test_the_originals_come_back_after_an_exception():
    real = (torch.empty, torch.empty_like)
    with pytest.raises(ZeroDivisionError):
        with da.dirty(0x40, CPU):
            assert torch.empty is not real[0]
            1 / 0
    assert (torch.empty, torch.empty_like) == real
    with pytest.raises(da.DirtyFailure):
        da.check("toy", lambda: op_skips_the_last_element(X), CPU, 1)
    assert (torch.empty, torch.empty_like) == real


class _Toy(torch.autograd.Function):
    """Allocates in forward and in backward, as the wrappers' Functions do."""

    @staticmethod
    def forward(ctx, x):
        out = torch.empty_like(x)
        out.copy_(x * x)
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        gx = torch.empty(tuple(x.shape), dtype=x.dtype, device=x.device)
        gx.copy_(2 * x * g)
        return gx


def test_a_correct_op_and_an_autograd_function_pass_under_every_fill():
    base = da.check("correct toy", lambda: op_correct(X), CPU, 3)
    assert [n for n, _ in base] == ["[0]", "[1]"] and torch.equal(base[1][1], X.max())

    def through_autograd():
        x = X.clone().requires_grad_(True)
        y = _Toy.apply(x)
        (g,) = torch.autograd.grad(y, x, torch.ones_like(y))
        return {"y": y.detach(), "g": g}
    base = da.check("autograd toy", through_autograd, CPU, 2)
    assert torch.equal(dict(base)["['g']"], 2 * X)


# ---- the planted defects ------------------------------------------------------------------------------------------------------------------------------------
def test_an_unwritten_output_element_is_reported():
    with pytest.raises(da.DirtyFailure, match=r"fill 0xFF against 0x00: result \(3, 5, 7\) holds 1 NaN the 0x00 run does not, first at \(2, 4, 6\)"):
        da.check("skips the last element", lambda: op_skips_the_last_element(X), CPU, 1)


def test_scratch_that_is_added_into_without_clearing_is_reported():
    with pytest.raises(da.DirtyFailure, match=r"fill 0xFF against 0x00: result \(3, 5, 7\) holds 105 NaN the 0x00 run does not, first at \(0, 0, 0\)"):
        da.check("uncleared scratch", lambda: op_adds_into_uncleared_scratch(X), CPU, 2)
    (zero, _), (finite, _) = _under(0x00, op_adds_into_uncleared_scratch), _under(0x40, op_adds_into_uncleared_scratch)
    assert not torch.equal(zero, finite) and bool(torch.isfinite(finite).all())


def test_a_maximum_against_an_unwritten_word_passes_under_ff_and_fails_under_40():
    zero, nan, finite = (_under(fill, op_max_against_an_unwritten_word)[0] for fill in da.FILLS)
    assert torch.equal(zero, X.max()) and torch.equal(nan, zero)          # the NaN vanished in the maximum: 0xFF alone sees nothing
    assert not torch.equal(finite, zero) and float(finite) == 3.00392150878906250
    with pytest.raises(da.DirtyFailure, match="fill 0x40 against 0x00: result"):
        da.check("max against an unwritten word", lambda: op_max_against_an_unwritten_word(X), CPU, 2)


def test_a_store_past_the_payload_is_reported():
    for fill in da.FILLS:
        out, d = _under(fill, op_writes_one_element_past_its_payload)
        assert torch.equal(out, X.reshape(-1)) and not d.guards_intact() and d.touched() == [(0, (105,), torch.float32)]
    with pytest.raises(da.DirtyFailure, match="fill 0x00: a byte outside the payload was written"):
        da.check("writes past its payload", lambda: op_writes_one_element_past_its_payload(X), CPU, 1)
    # ... and one in front of it
    with da.dirty(0xFF, CPU) as d:
        out = torch.empty(8, dtype=torch.float32, device="cpu")
        out.zero_()
        out.as_strided((1,), (1,), out.storage_offset() - 1).zero_()
    assert not d.guards_intact()


def test_a_run_that_intercepts_nothing_is_reported():
    def allocates_elsewhere():
        return torch.zeros(3) + X.sum()
    with pytest.raises(da.DirtyFailure, match="0 allocations intercepted, the wrapper makes at least 1"):
        da.check("sees nothing", allocates_elsewhere, CPU, 1)
    with pytest.raises(da.DirtyFailure, match="3 allocations intercepted, the wrapper makes at least 4"):
        da.check("sees too few", lambda: op_correct(X), CPU, 4)


def test_the_caches_are_emptied_before_every_run():
    calls = []
    da.check("counts", lambda: op_correct(X), CPU, 3, before=lambda: calls.append(1))
    assert len(calls) == 1 + len(da.FILLS)


# ---- the wrappers allocate through what the harness replaces, and through nothing else ------------------------------------------------------------------
def _code(path):
    """The module's code without strings and comments: its tokens one blank apart, dotted names and the bracket of a call closed up."""
    with open(path) as f:
        text = f.read()
    keep = (tokenize.NAME, tokenize.OP, tokenize.NUMBER)
    code = " ".join(tok.string for tok in tokenize.generate_tokens(io.StringIO(text).readline) if tok.type in keep)
    return re.sub(r" \(", "(", re.sub(r" ?\. ?", ".", code))


@pytest.mark.parametrize("module", WRAPPERS)
def test_the_wrappers_allocate_through_torch_empty_only(module):
    code = _code(os.path.join(ROOT, "ibgs_amd", module))
    spelled = re.findall(r"[\w.]*empty\w*\(?", code)
    assert spelled and set(spelled) <= {"torch.empty(", "torch.empty_like("}, (module, sorted(set(spelled)))
    code = code.replace("from torch import nn ", "")          # (the one name the wrappers import from torch)
    for other in ("new_empty", "empty_strided", "empty_permuted", "Tensor(", ".new(", "FloatTensor", "ByteTensor", "HalfTensor", "DoubleTensor", "IntTensor", "import torch as",
                  "from torch import"):
        assert other not in code, (module, other)
