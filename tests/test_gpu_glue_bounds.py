"""Buffer ends of the three fused glue units (depth_normal.hip, loss.hip, activate.hip), through their C entry points: every array sits inside a larger
allocation (tests/glue_edges.py `Guarded`).  Around an OUTPUT, 64 KiB of guard words each side must come back unchanged (an int32 comparison); around an
INPUT the same padding is NaN, so a read past either end that reaches a result shows up in it: every result must be finite and equal, bit for bit, the run on
plain buffers.  An output's payload starts as another NaN pattern: a finite result was written.

Activations as well: every non-empty subset of (scale, rotation, opacity), forward and backward, gives the bits of the all-three run and leaves the other
buffers alone, and the calls the entry points must refuse are refused before anything is launched.

Every call writes inside memory this file allocated; nothing here is meant to fault."""
import itertools

import pytest
import torch

from ibgs_amd import _lib
from tests import glue_edges as ge
from tests.glue_edges import Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _finite_bits(g):
    assert torch.isfinite(g.view).all(), "a result holds a NaN / inf: never written, or computed from a read past an input's end"
    return g.bits()


def _all_intact(*bufs):
    torch.cuda.synchronize()
    return all(b.guards_intact() for b in bufs)


# ---- depth -> normal ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["65x9", "63x7", "2x2", "197x29"])
def test_depth_normal_buffer_ends(case):
    lib = _lib.load()
    r = ge.reference(case)
    W, H, k = r.W, r.H, (r.cam.Fx, r.cam.Fy, r.cam.Cx, r.cam.Cy)
    depth, cot = r.depth.to(DEV).contiguous(), r.cot.to(DEV).contiguous()
    plain_n, plain_g = torch.full((3, H, W), float("nan"), device=DEV), torch.full((H, W), float("nan"), device=DEV)
    assert lib.ibgs_depth_normal_forward(_stream(), W, H, *k, depth.data_ptr(), plain_n.data_ptr()) == 0
    assert lib.ibgs_depth_normal_backward(_stream(), W, H, *k, depth.data_ptr(), cot.data_ptr(), plain_g.data_ptr()) == 0
    gd, gc = Guarded(H * W, depth), Guarded(3 * H * W, cot)
    gn, gg = Guarded(3 * H * W), Guarded(H * W)
    assert lib.ibgs_depth_normal_forward(_stream(), W, H, *k, gd.ptr(), gn.ptr()) == 0
    assert lib.ibgs_depth_normal_backward(_stream(), W, H, *k, gd.ptr(), gc.ptr(), gg.ptr()) == 0
    assert _all_intact(gn, gg) and gd.untouched() and gc.untouched()
    assert torch.equal(_finite_bits(gn), plain_n.view(torch.int32).reshape(-1))
    assert torch.equal(_finite_bits(gg), plain_g.view(torch.int32).reshape(-1))


# ---- L1 -----------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 5, 4097])
@pytest.mark.parametrize("shift", [0, 1])
def test_l1_buffer_ends(n, shift):
    """shift 1: every array four bytes off 16-byte alignment (the scalar loops); 0: the float4 bodies and their tails."""
    lib = _lib.load()
    gen = torch.Generator(device=DEV).manual_seed(n)
    a, b = torch.rand(n, device=DEV, generator=gen), torch.rand(n, device=DEV, generator=gen)
    sc = torch.empty(lib.ibgs_required_l1(), dtype=torch.uint8, device=DEV)
    w = torch.tensor([0.75], device=DEV)

    def run(x, y, g, g2, loss):
        assert lib.ibgs_l1_loss(_stream(), n, x, y, g, loss, sc.data_ptr(), sc.numel()) == 0
        assert lib.ibgs_l1_grad(_stream(), n, x, y, w.data_ptr(), g2) == 0
        assert lib.ibgs_l1_rescale(_stream(), n, g, w.data_ptr()) == 0

    pa, pb, pg, pg2, pl = Guarded(n, a, shift=shift), Guarded(n, b, shift=shift), Guarded(n, shift=shift), Guarded(n, shift=shift), Guarded(1)
    run(pa.ptr(), pb.ptr(), pg.ptr(), pg2.ptr(), pl.ptr())
    assert _all_intact(pg, pg2, pl) and pa.untouched() and pb.untouched()
    assert pa.ptr() % 16 == 4 * shift
    # the same on plain buffers of exactly n words (as the wrapper allocates them)
    qa, qb, qg, qg2, ql = a.clone(), b.clone(), torch.full((n,), float("nan"), device=DEV), torch.full((n,), float("nan"), device=DEV), torch.full((1,), float("nan"), device=DEV)
    run(qa.data_ptr(), qb.data_ptr(), qg.data_ptr(), qg2.data_ptr(), ql.data_ptr())
    for got, want in ((pg, qg), (pg2, qg2), (pl, ql)):
        assert torch.equal(_finite_bits(got), want.view(torch.int32))
    assert torch.equal(pg.bits(), pg2.bits())             # loss + rescale = the one-pass gradient


# ---- activations --------------------------------------------------------------------------------------------------------------------------------------

def _raw(P, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    s = torch.randn(P, 3, device=DEV, generator=g) * 1.5 - 3.0
    r = torch.randn(P, 4, device=DEV, generator=g)
    o = torch.randn(P, 1, device=DEV, generator=g) * 3.0
    r[0] = 0.0          # the clamp of F.normalize
    return s, r, o, torch.randn(P, 3, device=DEV, generator=g), torch.randn(P, 4, device=DEV, generator=g), torch.randn(P, 1, device=DEV, generator=g)


WIDTH = (3, 4, 1)
SUBSETS = [c for c in itertools.product((False, True), repeat=3) if any(c)]


def _plain_activations(lib, P, raw, gin):
    outs = [torch.full((P, w), float("nan"), device=DEV) for w in WIDTH]
    douts = [torch.full((P, w), float("nan"), device=DEV) for w in WIDTH]
    assert lib.ibgs_activate_forward(_stream(), P, *[t.data_ptr() for t in raw], *[t.data_ptr() for t in outs]) == 0
    assert lib.ibgs_activate_backward(_stream(), P, *[t.data_ptr() for t in raw], *[t.data_ptr() for t in gin], *[t.data_ptr() for t in douts]) == 0
    torch.cuda.synchronize()
    assert all(torch.isfinite(t).all() for t in outs + douts)
    return [t.view(torch.int32).reshape(-1) for t in outs], [t.view(torch.int32).reshape(-1) for t in douts]


@pytest.mark.parametrize("P", [1, 63, 64, 65, 255, 256, 257])
def test_activation_buffer_ends(P):
    lib = _lib.load()
    data = _raw(P, P)
    raw, gin = data[:3], data[3:]
    want_f, want_b = _plain_activations(lib, P, raw, gin)
    graw, ggin = [Guarded(P * w, t) for w, t in zip(WIDTH, raw)], [Guarded(P * w, t) for w, t in zip(WIDTH, gin)]
    gout, gdout = [Guarded(P * w) for w in WIDTH], [Guarded(P * w) for w in WIDTH]
    assert lib.ibgs_activate_forward(_stream(), P, *[g.ptr() for g in graw], *[g.ptr() for g in gout]) == 0
    assert lib.ibgs_activate_backward(_stream(), P, *[g.ptr() for g in graw], *[g.ptr() for g in ggin], *[g.ptr() for g in gdout]) == 0
    assert _all_intact(*gout, *gdout) and all(g.untouched() for g in graw + ggin)
    for got, want in zip(gout + gdout, want_f + want_b):
        assert torch.equal(_finite_bits(got), want)


@pytest.mark.parametrize("P", [65, 257])
@pytest.mark.parametrize("subset", SUBSETS, ids=lambda c: "".join(n for n, on in zip("sro", c) if on))
def test_activation_subsets(P, subset):
    lib = _lib.load()
    data = _raw(P, 7 * P)
    raw, gin = data[:3], data[3:]
    want_f, want_b = _plain_activations(lib, P, raw, gin)
    sel = lambda ptrs: [p if on else None for p, on in zip(ptrs, subset)]
    rp, gp = [t.data_ptr() for t in raw], [t.data_ptr() for t in gin]
    # forward: only the chosen inputs are given; every output buffer is (a given output without its input is legal and must stay as it was)
    for give_all_outputs in (True, False):
        out = [Guarded(P * w) for w in WIDTH]
        op = [g.ptr() for g in out]
        assert lib.ibgs_activate_forward(_stream(), P, *sel(rp), *(op if give_all_outputs else sel(op))) == 0
        assert _all_intact(*out)
        for g, want, on in zip(out, want_f, subset):
            assert torch.equal(_finite_bits(g), want) if on else g.untouched()
    # backward: the chosen outputs, with every input given and with only theirs
    for give_all_inputs in (True, False):
        dout = [Guarded(P * w) for w in WIDTH]
        dp = sel([g.ptr() for g in dout])
        assert lib.ibgs_activate_backward(_stream(), P, *(rp if give_all_inputs else sel(rp)), *(gp if give_all_inputs else sel(gp)), *dp) == 0
        assert _all_intact(*dout)
        for g, want, on in zip(dout, want_b, subset):
            assert torch.equal(_finite_bits(g), want) if on else g.untouched()


def test_activation_calls_that_must_be_refused():
    lib, P = _lib.load(), 65
    data = _raw(P, 11)
    rp, gp = [t.data_ptr() for t in data[:3]], [t.data_ptr() for t in data[3:]]
    out, dout = [Guarded(P * w) for w in WIDTH], [Guarded(P * w) for w in WIDTH]
    op, dp = [g.ptr() for g in out], [g.ptr() for g in dout]

    def refused(rc, text):
        assert rc < 0
        assert text in _lib.last_error(), _lib.last_error()
        assert lib.ibgs_l1_loss(None, 0, None, None, None, None, None, 0) < 0 and "ibgs_l1_loss" in _lib.last_error()          # another message in between: the next one is fresh
        torch.cuda.synchronize()
        assert all(g.untouched() for g in out + dout)          # nothing was launched

    refused(lib.ibgs_l1_loss(None, 0, None, None, None, None, None, 0), "ibgs_l1_loss")
    for i in range(3):          # an input without its output
        o = list(op); o[i] = None
        refused(lib.ibgs_activate_forward(_stream(), P, *rp, *o), "activate: ")
    for i in range(3):          # a backward output without its raw input, without its incoming gradient
        r = list(rp); r[i] = None
        refused(lib.ibgs_activate_backward(_stream(), P, *r, *gp, *dp), "activate backward: ")
        g = list(gp); g[i] = None
        refused(lib.ibgs_activate_backward(_stream(), P, *rp, *g, *dp), "activate backward: ")
    refused(lib.ibgs_activate_forward(_stream(), -1, *rp, *op), "activate: ")
    refused(lib.ibgs_activate_backward(_stream(), -1, *rp, *gp, *dp), "activate backward: ")
    # and P = 0 is a valid empty call
    assert lib.ibgs_activate_forward(_stream(), 0, *rp, *op) == 0 and lib.ibgs_activate_backward(_stream(), 0, *rp, *gp, *dp) == 0
    torch.cuda.synchronize()
    assert all(g.untouched() for g in out + dout)
