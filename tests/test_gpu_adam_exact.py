"""The optimiser kernels (adam_kernel, adam_sh_kernel, sh_grad_from_views_kernel) against tests/adam_ref.py, the numpy restatement of adam_math.h's contract:
parameters and both moments equal to the restatement as bytes after every step, in the regimes where a wrong formula shows (small parameters, denominators at
eps, zero gradients on live moments, large step counts, overflow), at the edges of the dispatch table and of the vector path, and with every written tensor
inside a sentinel-filled buffer.  The restatement itself is checked on the CPU in tests/test_adam_host.py."""
import ctypes
import math

import numpy as np
import pytest
import torch

from ibgs_amd import _lib
from ibgs_amd.optim import FusedAdam
from ibgs_amd.shgrad import sh_grad_from_views
from tests import adam_ref
from tests.metrics import rel_l2
from tests.test_gpu_anisotropic import F64_K

pytestmark = pytest.mark.gpu
BETAS, EPS = (0.9, 0.999), 1e-15          # the reference's Adam (scene/gaussian_model.py:241)
STEPS = 12
f32 = np.float32


def host(t):
    return t.detach().cpu().numpy().copy()


def dev(a):
    return torch.from_numpy(np.array(a, f32)).cuda()


def assert_bits(got, want, what):
    """Equal as bytes (so -0 is not +0 and a NaN is its own payload); names the first element that differs."""
    a = np.ascontiguousarray(host(got) if torch.is_tensor(got) else got, f32).reshape(-1)
    b = np.ascontiguousarray(want, f32).reshape(-1)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    ua, ub = a.view(np.uint32), b.view(np.uint32)
    if not np.array_equal(ua, ub):
        bad = np.flatnonzero(ua != ub)
        i = int(bad[0])
        raise AssertionError("%s: %d of %d elements differ; first at %d: device %r (0x%08x), restatement %r (0x%08x)"
                             % (what, bad.size, a.size, i, float(a[i]), int(ua[i]), float(b[i]), int(ub[i])))


class Mirror:
    """One tensor's parameter, moments and step count, carried by the restatement."""

    def __init__(self, p, lr, m=None, v=None, t=0):
        self.p = np.array(p, f32)
        self.m = np.zeros_like(self.p) if m is None else np.array(m, f32)
        self.v = np.zeros_like(self.p) if v is None else np.array(v, f32)
        self.t, self.lr, self.parts = t, lr, {}

    def step(self, g):
        self.t += 1
        self.p, self.m, self.v = adam_ref.adam_step(self.p, g, self.m, self.v, self.t, self.lr, BETAS, EPS, f32, self.parts)

    def check(self, opt, param, what):
        st = opt.state[param]
        assert float(st["step"]) == self.t, (what, float(st["step"]), self.t)
        assert_bits(st["exp_avg"], self.m, what + " exp_avg")
        assert_bits(st["exp_avg_sq"], self.v, what + " exp_avg_sq")
        assert_bits(param, self.p, what + " param")


def mixed_params(rng, shape):
    """A third zeros, a third ~1e-6, a third O(1): on the first two the update (lr x O(1)) is far above the parameter's own rounding."""
    p = rng.standard_normal(shape).astype(f32)
    kind = rng.integers(0, 3, shape)
    p[kind == 0] = 0.0
    p[kind == 1] *= f32(1e-6)
    return p


def make_optim(params_np, lrs):
    params = [torch.nn.Parameter(dev(p)) for p in params_np]
    opt = FusedAdam([{"params": [p], "lr": lr} for p, lr in zip(params, lrs)], lr=0.0, eps=EPS)
    return params, opt, [Mirror(p, lr) for p, lr in zip(params_np, lrs)]


def run_steps(params, opt, mirrors, grads_of, what, steps=STEPS):
    """grads_of(it, j) -> numpy gradient of tensor j on step it, or None (skipped)."""
    for it in range(steps):
        for j, (p, mir) in enumerate(zip(params, mirrors)):
            g = grads_of(it, j)
            p.grad = None if g is None else dev(g)
            if g is not None:
                mir.step(np.asarray(g, f32))
        opt.step()
        torch.cuda.synchronize()
        for j, (p, mir) in enumerate(zip(params, mirrors)):
            mir.check(opt, p, "%s, step %d, tensor %d %s" % (what, it + 1, j, tuple(p.shape)))


# ---- (a) the arithmetic, to the bit ---------------------------------------------------------------------------------------------------------------------------
SHAPES = [(5003, 3), (1237,), (130, 15, 3), (777, 4)]
LRS = [1.6e-4, 1e-2, 1.25e-4, 5e-2]


def test_ordinary_gradients_bit_for_bit():
    rng = np.random.default_rng(21)
    start = [mixed_params(rng, s) for s in SHAPES]
    params, opt, mirrors = make_optim(start, LRS)
    run_steps(params, opt, mirrors, lambda it, j: rng.standard_normal(SHAPES[j]).astype(f32) * f32(10.0 ** ((it % 5) - 3)), "ordinary")
    for mir, p0 in zip(mirrors, start):          # the update is resolved: where the parameter started at zero, nothing but the twelve steps is there
        assert (p0 == 0).mean() > 0.3 and np.all(mir.p[p0 == 0] != 0)


def eps_regime_exponents(rng, shape):
    """Every element keeps its magnitude 10^e over the steps, as a Gaussian that reaches almost no pixel does: three fifths with e in [-16.5, -13.5], so that
    sqrt(v_hat) ~ |g| lies within a decade and a half of eps = 1e-15, the rest with e in [-24, -12]: (1 - b2) g^2 is subnormal below |g| = 3.4e-18 and zero
    below 1.2e-21, while m ~ 0.1 g stays a normal number."""
    return np.where(rng.random(shape) < 0.6, rng.uniform(-16.5, -13.5, shape), rng.uniform(-24.0, -12.0, shape))


def eps_regime_gradients(rng, e, it):
    """+-10^e times a factor in [0.5, 2); from the second step on a fifth of the gradients are exactly zero, on elements whose moments the first step made non-zero."""
    g = (np.where(rng.random(e.shape) < 0.5, -1.0, 1.0) * rng.uniform(0.5, 2.0, e.shape) * 10.0 ** e).astype(f32)
    if it > 0:
        g[rng.random(e.shape) < 0.2] = 0.0
    return g


def test_eps_regime_bit_for_bit():
    rng = np.random.default_rng(22)
    shapes, lrs = [(4099, 3), (1237,)], [1.6e-4, 5e-2]
    expo = [eps_regime_exponents(rng, s) for s in shapes]
    grads = [[eps_regime_gradients(rng, e, it) for e in expo] for it in range(STEPS)]
    # on the restatement alone: the regime is the one this test is about
    for j, s in enumerate(shapes):
        mir = Mirror(np.zeros(s, f32), lrs[j])
        at_eps, tiny_v, zero_g_live = np.zeros(s, bool), np.zeros(s, bool), np.zeros(s, bool)
        for it in range(STEPS):
            live = (mir.m != 0) & (mir.v != 0)
            mir.step(grads[it][j])
            scaled = mir.parts["scaled"].astype(np.float64)
            at_eps |= (scaled >= 0.1 * EPS) & (scaled <= 10 * EPS)
            tiny_v |= (mir.v < np.finfo(f32).tiny) & (mir.m != 0)
            zero_g_live |= live & (grads[it][j] == 0)
        print("[adam eps] %s: sqrt(v) / sqrt(bc2) within a decade of eps on %.1f %% of the elements, v subnormal or zero beside a live m on %.1f %%, "
              "a zero gradient on live moments on %.1f %%" % (s, 100 * at_eps.mean(), 100 * tiny_v.mean(), 100 * zero_g_live.mean()))
        assert at_eps.mean() >= 0.25 and tiny_v.any() and zero_g_live.mean() >= 0.15
        assert ((mir.v > 0) & (mir.v < np.finfo(f32).tiny)).any() and ((mir.v == 0) & (mir.m != 0)).any()
    params, opt, mirrors = make_optim([mixed_params(rng, s) for s in shapes], lrs)
    run_steps(params, opt, mirrors, lambda it, j: grads[it][j], "eps regime")


def test_step_counts_bit_for_bit():
    """Different step counts in one launch, one of them past the underflow of b1^t; a tensor that is skipped on some steps keeps its count."""
    rng = np.random.default_rng(23)
    counts = [1, 2, 1000, 100000, 0]
    shapes = [(1237,), (777, 4), (4099, 3), (130, 15, 3), (515,)]
    lrs = [1e-2, 5e-2, 1.6e-4, 1.25e-4, 1e-3]
    params_np = [mixed_params(rng, s) for s in shapes]
    params = [torch.nn.Parameter(dev(p)) for p in params_np]
    opt = FusedAdam([{"params": [p], "lr": lr} for p, lr in zip(params, lrs)], lr=0.0, eps=EPS)
    mirrors = []
    for p, pn, lr, t, s in zip(params, params_np, lrs, counts, shapes):
        m = (rng.standard_normal(s) * 1e-2).astype(f32) if t else np.zeros(s, f32)
        v = ((rng.standard_normal(s) * 1e-2) ** 2).astype(f32) if t else np.zeros(s, f32)
        opt.state[p] = {"step": torch.tensor(float(t)), "exp_avg": dev(m), "exp_avg_sq": dev(v)}
        mirrors.append(Mirror(pn, lr, m, v, t))

    def grads_of(it, j):
        if j == 4 and it in (0, 3, 4):
            return None
        return rng.standard_normal(shapes[j]).astype(f32) * f32(10.0 ** ((it % 5) - 3))
    run_steps(params, opt, mirrors, grads_of, "step counts")
    assert [m.t for m in mirrors] == [13, 14, 1012, 100012, 9]
    assert math.pow(0.9, 100001.0) == 0.0


def test_huge_gradients_bit_for_bit():
    """(1 - b2) g g is finite at |g| = 1e19 and 1e20 and infinite from 1e21 on: there sqrt(v) = inf, m / inf = 0 and the parameter stays, for good (b2 inf = inf)."""
    rng = np.random.default_rng(24)
    s = (2051,)
    mags = np.array([1e19, 1e20, 1e21, 1e25], f32)[rng.integers(0, 4, s)]
    sign = np.where(rng.random(s) < 0.5, -1.0, 1.0).astype(f32)
    params, opt, mirrors = make_optim([mixed_params(rng, s)], [1e-2])
    p0 = mirrors[0].p.copy()

    def grads_of(it, j):
        if it < 3:
            return mags * sign * f32(1.0 + 0.25 * it)
        return rng.standard_normal(s).astype(f32)
    run_steps(params, opt, mirrors, grads_of, "huge gradients", steps=6)
    inf = np.isinf(mirrors[0].v)
    assert np.array_equal(inf, mags > 5e20) and inf.any() and (~inf).any()
    assert np.array_equal(mirrors[0].p[inf], p0[inf]) and np.all(mirrors[0].p[~inf] != p0[~inf])
    assert np.isfinite(mirrors[0].p).all() and np.isfinite(mirrors[0].m).all()


# ---- (b) dispatch and bounds ------------------------------------------------------------------------------------------------------------------------------------
GUARD = 64          # floats of sentinel on either side of every view (256 B: the views start 16-byte aligned when the offset is 0)
SENTINEL = f32(-7.25e11)
ROLES = ("param", "grad", "exp_avg", "exp_avg_sq")


class Guarded:
    """n floats inside a sentinel-filled buffer, `off` floats (4 bytes each) past a 16-byte boundary."""

    def __init__(self, values, off):
        values = np.asarray(values, f32).reshape(-1)
        self.n, self.start = values.size, GUARD + off
        self.buf = torch.full((2 * GUARD + 4 + self.n,), float(SENTINEL), device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.view = self.buf[self.start:self.start + self.n]
        self.view.copy_(dev(values))
        assert self.n == 0 or self.view.data_ptr() % 16 == 4 * off

    def intact(self):
        b = host(self.buf)
        return bool(np.all(b[:self.start] == SENTINEL) and np.all(b[self.start + self.n:] == SENTINEL))


def guarded_run(sizes, offs, seed, what, steps=3, lr_of=lambda j: LRS[j % 4]):
    """One FusedAdam over 1-D tensors of `sizes` elements, every parameter, gradient and moment a view placed offs[j][role] floats off alignment; checks the
    restatement's bits and the sentinels after every step and returns the final (param, exp_avg, exp_avg_sq) of every tensor."""
    rng = np.random.default_rng(seed)
    ten, mirrors = [], []
    for j, n in enumerate(sizes):
        pn = mixed_params(rng, (n,))
        g = {r: Guarded(pn if r == "param" else np.zeros(n, f32), offs[j].get(r, 0)) for r in ROLES}
        g["p"] = torch.nn.Parameter(g["param"].view)
        assert g["p"].data_ptr() == g["param"].view.data_ptr()
        ten.append(g); mirrors.append(Mirror(pn, lr_of(j)))
    opt = FusedAdam([{"params": [g["p"]], "lr": lr_of(j)} for j, g in enumerate(ten)], lr=0.0, eps=EPS)
    for g in ten:
        opt.state[g["p"]] = {"step": torch.tensor(0.0), "exp_avg": g["exp_avg"].view, "exp_avg_sq": g["exp_avg_sq"].view}
    for it in range(steps):
        grads = [rng.standard_normal(n).astype(f32) * f32(10.0 ** ((it % 5) - 3)) for n in sizes]
        for g, mir, gr in zip(ten, mirrors, grads):
            g["grad"].view.copy_(dev(gr))
            g["p"].grad = g["grad"].view
            mir.step(gr)
        opt.step()
        torch.cuda.synchronize()
        for j, (g, mir) in enumerate(zip(ten, mirrors)):
            tag = "%s, step %d, tensor %d of %d elements, offsets %s" % (what, it + 1, j, g["param"].n, offs[j])
            st = opt.state[g["p"]]
            assert st["exp_avg"].data_ptr() == g["exp_avg"].view.data_ptr() and st["exp_avg_sq"].data_ptr() == g["exp_avg_sq"].view.data_ptr(), tag
            mir.check(opt, g["p"], tag)
            for r in ROLES:
                assert g[r].intact(), tag + ": the kernel wrote outside " + r
            assert_bits(g["grad"].view, grads[j], tag + " grad (read-only)")
    return [(mir.p, mir.m, mir.v) for mir in mirrors]


def test_chunk_edges_and_an_empty_tensor_in_one_launch():
    """adam_kernel's table: 4096 elements per workgroup, `first_block` per tensor; an empty tensor takes no entry."""
    sizes = [1, 3, 4, 5, 4095, 4096, 4097, 8191, 8192, 8193]
    order = np.random.default_rng(31).permutation(len(sizes))
    sizes = [sizes[i] for i in order]
    sizes.insert(5, 0)
    assert len(sizes) == 11 and sizes[5] == 0
    guarded_run(sizes, [{}] * len(sizes), 32, "chunk edges")


@pytest.mark.parametrize("n_tensors", [16, 17, 33])
def test_more_tensors_than_one_launch_holds(n_tensors):
    """FusedAdam.step passes 16 tensors per launch (IBGS_ADAM_MAX_TENSORS)."""
    pool = [1237, 4096, 5, 4097, 130, 1, 8193, 64, 3001]
    guarded_run([pool[j % len(pool)] + j for j in range(n_tensors)], [{}] * n_tensors, 33 + n_tensors, "%d tensors" % n_tensors, steps=2)


def test_every_pointer_off_alignment_takes_the_scalar_path_to_the_same_bytes():
    """Each of the four pointers in turn 4, 8 and 12 bytes past a 16-byte boundary, at element counts that are and are not multiples of 4, below and above
    one workgroup's chunk; against the restatement (inside guarded_run) and against the same data run aligned."""
    counts = [8, 5, 4100, 4099]
    sizes, offs = [], []
    for r in ROLES:
        for off in (1, 2, 3):
            for n in counts:
                sizes.append(n); offs.append({r: off})
    sizes += counts; offs += [{r: 3 - i for i, r in enumerate(ROLES)}] * 4          # and all four at once, differently
    shifted = guarded_run(sizes, offs, 35, "misaligned", steps=3)
    aligned = guarded_run(sizes, [{}] * len(sizes), 35, "aligned twin", steps=3)
    for j, (a, b) in enumerate(zip(shifted, aligned)):
        for x, y, name in zip(a, b, ("param", "exp_avg", "exp_avg_sq")):
            assert_bits(x, y, "tensor %d %s: misaligned against aligned" % (j, name))


# ---- (d) the SH coefficients straight from the factors ------------------------------------------------------------------------------------------------------------
SH_LRS = (2.5e-3, 1.25e-4)


def sh_factors(rng, P, V, it, pad):
    """means (P, 3), camposes (V, 3), dcolor (V, P, 3) as a view with row stride 3 P + pad; a seventh of the Gaussians (3, 10, ...) reached no pixel in any view."""
    means = (rng.standard_normal((P, 3)) * 3.0).astype(f32)
    cams = (rng.standard_normal((V, 3)) * 5.0 + 9.0).astype(f32)
    dc = (rng.standard_normal((V, P, 3)) * 10.0 ** (it - 2)).astype(f32)
    dc[:, 3::7] = 0.0
    buf = torch.full((V, 3 * P + pad), float("nan"), device="cuda")
    view = buf[:, :3 * P].unflatten(1, (P, 3))
    view.copy_(dev(dc))
    assert view.shape == (V, P, 3) and (V == 1 or view.stride() == (3 * P + pad, 3, 1))
    return means, cams, dc, view


def sh_case(P, M, Ks, degrees, V, via_abi=False, pad=0, off=0, seed=41):
    """Coefficient tensors of Ks coefficients each (in coefficient order, summing to M) stepped from the factors, one step per entry of `degrees`, against
    adam_step_sh on the device's own sh_grad_from_views output.  off: floats past a 16-byte boundary for every parameter and moment (in a sentinel buffer)."""
    rng = np.random.default_rng(seed)
    assert sum(Ks) == M and (via_abi or pad == 0)
    k0s = [sum(Ks[:j]) for j in range(len(Ks))]
    lib = _lib.load()
    xyz = torch.nn.Parameter(torch.zeros(P, 3, device="cuda"))
    mirrors, bufs, params = [], [], []
    for j, K in enumerate(Ks):
        pn = mixed_params(rng, (P, K, 3))
        g = {r: Guarded(pn if r == "param" else np.zeros(pn.size, f32), off) for r in ("param", "exp_avg", "exp_avg_sq")}
        bufs.append(g)
        params.append(torch.nn.Parameter(g["param"].view.view(P, K, 3)))
        mirrors.append(Mirror(pn, SH_LRS[j]))
    opt = FusedAdam([{"params": [xyz], "lr": 1.6e-4}] + [{"params": [p], "lr": SH_LRS[j]} for j, p in enumerate(params)], lr=0.0, eps=EPS)
    for p, g in zip(params, bufs):
        opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": g["exp_avg"].view.view(p.shape), "exp_avg_sq": g["exp_avg_sq"].view.view(p.shape)}
    for it, deg in enumerate(degrees):
        means, cams, dc, dview = sh_factors(rng, P, V, it, pad)
        xyz.data.copy_(dev(means))
        grad = host(sh_grad_from_views(xyz.detach(), dev(cams), dview, deg, M))
        before = [(m.p.copy(), m.m.copy()) for m in mirrors]
        new = adam_ref.adam_step_sh([(m.p, m.m, m.v) for m in mirrors], k0s, [m.t + 1 for m in mirrors], SH_LRS, grad=grad, betas=BETAS, eps=EPS, dtype=f32)
        for m, (p_, m_, v_) in zip(mirrors, new):
            m.p, m.m, m.v, m.t = p_, m_, v_, m.t + 1
        if via_abi:
            ds = []
            for p, g, m in zip(params, bufs, mirrors):
                d = _lib.AdamTensor()
                d.param, d.grad, d.exp_avg, d.exp_avg_sq = p.data_ptr(), None, g["exp_avg"].view.data_ptr(), g["exp_avg_sq"].view.data_ptr()
                d.numel, d.lr, d.beta1, d.beta2, d.eps = p.numel(), m.lr, BETAS[0], BETAS[1], EPS
                d.bias_correction1, d.bias_correction2 = 1.0 - math.pow(BETAS[0], float(m.t)), 1.0 - math.pow(BETAS[1], float(m.t))
                ds.append(d)
            arr = (_lib.AdamTensor * len(ds))(*ds)
            a0, aK = (ctypes.c_int32 * len(ds))(*k0s), (ctypes.c_int32 * len(ds))(*Ks)
            cams_d = dev(cams)
            rc = lib.ibgs_adam_step_sh(torch.cuda.current_stream().cuda_stream, P, deg, V, xyz.data_ptr(), cams_d.data_ptr(), dview.data_ptr(), 3 * P + pad,
                                       len(ds), ctypes.cast(arr, ctypes.c_void_p), ctypes.cast(a0, ctypes.c_void_p), ctypes.cast(aK, ctypes.c_void_p))
            assert rc == 0, _lib.last_error()
            for p in params:
                opt.state[p]["step"] += 1
        else:
            items = [{"dcolor": dview[v], "campos": dev(cams[v]), "degree": deg, "M": M} for v in range(V)]
            opt.step(sh_factors=items, sh_params=tuple(params), means3D=xyz)
        torch.cuda.synchronize()
        nb = (deg + 1) ** 2
        for j, (p, g, m) in enumerate(zip(params, bufs, mirrors)):
            tag = "P %d, M %d, Ks %s, degree %d, %d views, step %d, tensor %d" % (P, M, Ks, deg, V, it + 1, j)
            m.check(opt, p, tag)
            assert all(g[r].intact() for r in g), tag + ": written outside the tensor"
            dead = slice(max(nb - k0s[j], 0), None)          # this tensor's coefficients above the active degree: a zero gradient
            if it > 0 and before[j][1][:, dead].any():
                assert np.all(grad[:, k0s[j]:k0s[j] + Ks[j]][:, dead] == 0)
                live = before[j][1][:, dead] != 0
                assert np.all(np.abs(m.m[:, dead][live]) < np.abs(before[j][1][:, dead][live])), tag + ": the stale first moment decays"
                assert np.mean(m.p[:, dead][live] != before[j][0][:, dead][live]) > 0.5, tag + ": and still moves the parameter"
        assert_bits(xyz, means, "positions are only read")
    return mirrors


@pytest.mark.parametrize("M,Ks", [(1, (1,)), (4, (4,)), (9, (9,)), (16, (16,)), (4, (1, 3)), (9, (1, 8)), (16, (1, 15))])
@pytest.mark.parametrize("P,V", [(1, 1), (63, 2), (64, 5), (65, 1), (129, 2)])
def test_sh_step_from_factors_is_the_restatement(M, Ks, P, V):
    top = int(math.isqrt(M)) - 1
    degrees = (top, top, max(top - 1, 0), 0) if top else (0, 0, 0)          # the degree drops below what M holds: stale moments on a zero gradient
    sh_case(P, M, Ks, degrees, V)


@pytest.mark.parametrize("M,Ks", [(16, (5, 11)), (9, (8, 1))])
@pytest.mark.parametrize("P,V,pad", [(1, 2, 5), (63, 1, 5), (64, 2, 5), (65, 5, 0), (129, 5, 5)])
def test_sh_step_through_the_c_abi_with_other_splits_and_a_padded_view_stride(M, Ks, P, V, pad):
    top = int(math.isqrt(M)) - 1
    sh_case(P, M, Ks, (top, top - 1, 1, top), V, via_abi=True, pad=pad)


@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("M,Ks,P,via_abi", [(16, (1, 15), 129, False), (9, (9,), 65, False), (16, (5, 11), 64, True), (4, (1, 3), 63, False)])
def test_sh_step_with_tensors_off_alignment(off, M, Ks, P, via_abi):
    top = int(math.isqrt(M)) - 1
    shifted = sh_case(P, M, Ks, (top, top - 1, top), 2, via_abi=via_abi, pad=5 if via_abi else 0, off=off)
    aligned = sh_case(P, M, Ks, (top, top - 1, top), 2, via_abi=via_abi, pad=5 if via_abi else 0, off=0)
    for a, b in zip(shifted, aligned):
        assert_bits(a.p, b.p, "param"); assert_bits(a.m, b.m, "exp_avg"); assert_bits(a.v, b.v, "exp_avg_sq")


# ---- (e) sh_grad_from_views against float64 -----------------------------------------------------------------------------------------------------------------------
ARB_FLOOR = 1e-6          # the small floor of tests/test_gpu_anisotropic.py's colour check, where both distances are a few roundings
SHG_CASES = [(M, deg) for M in (1, 4, 9, 16) for deg in range(4) if (deg + 1) ** 2 <= M]
assert (16, 1) in SHG_CASES and len(SHG_CASES) == 10


@pytest.mark.parametrize("M,deg", SHG_CASES)
@pytest.mark.parametrize("P,V,pad", [(1, 1, 0), (63, 3, 5), (64, 8, 0), (65, 3, 0), (1000, 8, 5), (1000, 1, 0), (64, 3, 5)])
def test_sh_grad_from_views_against_float64(M, deg, P, V, pad):
    rng = np.random.default_rng(1000 * M + 100 * deg + P + V)
    means, cams, dc, dview = sh_factors(rng, P, V, 2, pad)
    if P > 3:
        assert not dc[:, 3].any() and dc[:, 1].any()
    got = host(sh_grad_from_views(dev(means), dev(cams), dview, deg, M))
    t64 = adam_ref.sh_grad_from_views(means, cams, dc, deg, M, np.float64)
    r32 = adam_ref.sh_grad_from_views(means, cams, dc, deg, M, f32)
    assert got.shape == (P, M, 3) and r32.dtype == f32
    nb = (deg + 1) ** 2
    assert not got[:, nb:].any(), "coefficients above the active degree are exact zeros"
    silent = ~dc.any(axis=(0, 2))
    assert not got[silent].any() and (silent.any() or P <= 3), "rows without any dL/dRGB are exact zeros"
    if not t64.any():
        assert not got.any()
        return
    e, floor = rel_l2(got, t64), rel_l2(r32, t64)
    print("[sh grad] M %d degree %d P %d views %d stride 3P+%d: relL2 vs float64 %.2e, fp32 restatement %.2e" % (M, deg, P, V, pad, e, floor))
    assert e <= max(ARB_FLOOR, F64_K * floor), (e, floor)
    # per coefficient as well: a wrong constant or sign in one basis function must not hide behind the others
    for k in range(nb):
        ek, fk = rel_l2(got[:, k], t64[:, k]), rel_l2(r32[:, k], t64[:, k])
        assert ek <= max(ARB_FLOOR, F64_K * fk), (k, ek, fk)


# ---- (f) a rejected step leaves the optimiser as it was ---------------------------------------------------------------------------------------------------------------
def split_sh_after_two_steps(seed=51):
    rng = np.random.default_rng(seed)
    P, M, Ks = 130, 16, (1, 15)
    xyz = torch.nn.Parameter(dev(rng.standard_normal((P, 3)) * 3.0))
    pn = [mixed_params(rng, (P, K, 3)) for K in Ks]
    params = [torch.nn.Parameter(dev(p)) for p in pn]
    opt = FusedAdam([{"params": [xyz], "lr": 1.6e-4}] + [{"params": [p], "lr": SH_LRS[j]} for j, p in enumerate(params)], lr=0.0, eps=EPS)
    mirrors = [Mirror(p, SH_LRS[j]) for j, p in enumerate(pn)]

    def good_step(it):
        cams = (rng.standard_normal((2, 3)) * 5.0 + 9.0).astype(f32)
        dc = dev(rng.standard_normal((2, P, 3)) * 0.1)
        grad = host(sh_grad_from_views(xyz.detach(), dev(cams), dc, 3, M))
        for m, k0, K in zip(mirrors, (0, 1), Ks):
            m.step(grad[:, k0:k0 + K])
        opt.step(sh_factors=[{"dcolor": dc[v], "campos": dev(cams[v]), "degree": 3, "M": M} for v in range(2)], sh_params=tuple(params), means3D=xyz)
        torch.cuda.synchronize()
        for j, (p, m) in enumerate(zip(params, mirrors)):
            m.check(opt, p, "valid step %d, tensor %d" % (it, j))
    good_step(1); good_step(2)
    item = {"dcolor": torch.full((P, 3), 0.25, device="cuda"), "campos": torch.zeros(3, device="cuda"), "degree": 3, "M": M}
    return xyz, params, opt, mirrors, item, good_step


def snapshot(opt, params):
    return [(float(opt.state[p]["step"]), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"], host(opt.state[p]["exp_avg"]), host(opt.state[p]["exp_avg_sq"]), host(p))
            for p in params]


@pytest.mark.parametrize("fault", ["dense grad on the second tensor", "second tensor of another optimiser", "second tensor not contiguous", "means3D of the wrong shape"])
def test_a_rejected_sh_step_leaves_the_optimiser_as_it_was(fault):
    xyz, params, opt, mirrors, item, good_step = split_sh_after_two_steps()
    snap = snapshot(opt, params)
    sh_params, means, exc = tuple(params), xyz, RuntimeError
    if fault.startswith("dense"):
        params[1].grad = torch.zeros_like(params[1])
    elif fault.startswith("second tensor of another"):
        sh_params, exc = (params[0], torch.nn.Parameter(params[1].detach().clone())), ValueError
    elif fault.startswith("second tensor not"):
        wide = torch.nn.Parameter(torch.zeros(130, 15, 6, device="cuda")[:, :, ::2])
        assert not wide.is_contiguous() and wide.shape == params[1].shape
        opt.add_param_group({"params": [wide], "lr": 1e-3})
        sh_params = (params[0], wide)
    else:
        means = torch.nn.Parameter(torch.zeros(131, 3, device="cuda"))
    with pytest.raises(exc):
        opt.step(sh_factors=[item], sh_params=sh_params, means3D=means)
    torch.cuda.synchronize()
    for p, (t, m_obj, v_obj, m_np, v_np, p_np) in zip(params, snap):
        st = opt.state[p]
        assert float(st["step"]) == t == 2.0, fault
        assert st["exp_avg"] is m_obj and st["exp_avg_sq"] is v_obj, fault
        assert_bits(st["exp_avg"], m_np, fault + ": exp_avg"); assert_bits(st["exp_avg_sq"], v_np, fault + ": exp_avg_sq"); assert_bits(p, p_np, fault + ": param")
    params[1].grad = None
    good_step(3)
    assert [m.t for m in mirrors] == [3, 3]


def test_a_failing_c_call_gives_the_step_counts_back():
    """The library refuses more than 3 degrees; by then the counts have moved, and they move back."""
    xyz, params, opt, mirrors, item, good_step = split_sh_after_two_steps()
    snap = snapshot(opt, params)
    with pytest.raises(RuntimeError, match="ibgs_adam_step_sh failed"):
        opt.step(sh_factors=[dict(item, degree=4)], sh_params=tuple(params), means3D=xyz)
    for p, (t, m_obj, v_obj, m_np, v_np, p_np) in zip(params, snap):
        st = opt.state[p]
        assert float(st["step"]) == t == 2.0
        assert_bits(st["exp_avg"], m_np, "exp_avg"); assert_bits(st["exp_avg_sq"], v_np, "exp_avg_sq"); assert_bits(p, p_np, "param")
    good_step(3)


def test_empty_sh_factors_skip_the_sh_tensors_like_a_missing_gradient():
    xyz, params, opt, mirrors, item, good_step = split_sh_after_two_steps()
    snap = snapshot(opt, params)
    x0 = host(xyz)
    xyz.grad = torch.ones_like(xyz)
    opt.step(sh_factors=[], sh_params=tuple(params), means3D=xyz)
    torch.cuda.synchronize()
    for p, (t, m_obj, v_obj, m_np, v_np, p_np) in zip(params, snap):
        st = opt.state[p]
        assert float(st["step"]) == 2.0 and st["exp_avg"] is m_obj and st["exp_avg_sq"] is v_obj
        assert_bits(st["exp_avg"], m_np, "exp_avg"); assert_bits(st["exp_avg_sq"], v_np, "exp_avg_sq"); assert_bits(p, p_np, "param")
    assert float(opt.state[xyz]["step"]) == 1.0 and (host(xyz) != x0).all()          # the dense tensors are stepped as usual
    xyz.grad = None
    good_step(3)
