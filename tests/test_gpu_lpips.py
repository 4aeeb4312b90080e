"""LPIPS on VGG16 (ibgs_amd.lpips; csrc/lpips.hip) on the device.

The ARBITER is tests/lpips_ref.forward_ref (float64 numpy).  The YARDSTICK of a tensor is d_ref = max(d_torch, d_chain): the max-abs distances from the arbiter
of tests/lpips_ref.torch_composition at float32 ON THE CPU and of tests/lpips_ref.chain_f32 (every convolution one k-ordered, singly rounded multiply-add chain
from the bias), on the same inputs.  THE BAR, as in tests/test_gpu_hourglass.py: for each of the ten tap tensors and five maps
max |hip - f64| <= F64_K x d_ref (F64_K = 2); where d_ref is exactly 0: 2^-22 max |f64|.  Every comparison prints its ratio before it asserts (DESIGN.md
section 17 quotes the range).  The scalar has no ratio of its own -- it is a mean of ~10^3 terms whose errors cancel, and a ratio of two such cancellations
is noise: |lpips - f64| <= 2 sum_k d_ref(map_k), and the returned scalar equals the float64 sum of the float64 means of the returned device maps, rounded once
to float32 (which pins the reduction).  Bit-for-bit properties are asserted with torch.equal.

The weights are `lpips_ref.seeded_params` (He-normal): the real VGG16 / LPIPS weights are not in the repository, and no value is pinned against the
reference's own run (DESIGN.md section 17 says what a user with the weights would run).  The kernel's tile side is 16: (17, 19) puts a pixel past a tile at
level 0, (33, 37) and (35, 50) at levels 0 and 1."""
import functools

import numpy as np
import pytest
import torch

from ibgs_amd import image_eval, lpips as lp
from tests import dirty_alloc as da
from tests import lpips_ref as ref

pytestmark = pytest.mark.gpu

F64_K = 2.0
FLOOR = 2.0 ** -22
FRAMES = [(16, 16), (17, 19), (33, 37), (35, 50), (16, 49), (49, 16)]
SEED = 5


# ---- parameters, inputs and the three CPU evaluations, computed once and shared: nobody writes them -----------------------------------------------------
@functools.lru_cache(maxsize=None)
def _params(kind):
    return ref.seeded_params(SEED, kind)


@functools.lru_cache(maxsize=None)
def _net(kind="default"):
    net = lp.LPIPSNet()
    net.load_state_dict({k: torch.tensor(v) for k, v in _params(kind).items()})
    return net.cuda()


@functools.lru_cache(maxsize=None)
def _pair(h, w):
    return ref.seeded_pair(100 * h + w, h, w)


@functools.lru_cache(maxsize=None)
def _cpu(h, w, kind):
    """-> (arbiter result, {item: d_ref}, {item: (d_torch, d_chain)})"""
    x, y = _pair(h, w)
    p = _params(kind)
    want = ref.forward_ref(x, y, p)
    t32, chain = ref.torch_composition(x, y, p, torch.float32), ref.chain_f32(x, y, p)
    both = {}
    for (name, a), (_, b), (_, c) in zip(ref.flat_items(want), ref.flat_items(t32), ref.flat_items(chain)):
        both[name] = (float(np.abs(b.numpy().astype(np.float64) - a).max()), float(np.abs(c.astype(np.float64) - a).max()))
    return want, {k: max(v) for k, v in both.items()}, both


def _dev(a):
    return torch.as_tensor(a).cuda()


def _check(name, got, want64, d, both):
    want = torch.as_tensor(np.asarray(want64), dtype=torch.float64, device=got.device)
    assert got.dtype == torch.float32 and got.shape == want.shape, (name, got.dtype, tuple(got.shape), tuple(want.shape))
    assert not bool(torch.isnan(got).any()), name
    err = float((got.double() - want).abs().max())
    print("%-28s err %.3e  d_ref %.3e (torch %.3e, chain %.3e)  ratio %s" % (name, err, d, both[0], both[1], "%.2f" % (err / d) if d > 0 else "-"))
    if d > 0:
        assert err <= F64_K * d, (name, err, d)
    else:
        assert err <= FLOOR * float(want.abs().max()), (name, err)


def _parity(h, w, kind):
    x, y = _pair(h, w)
    want, d_ref, both = _cpu(h, w, kind)
    value, maps, (fx, fy), taps = lp.lpips(_dev(x), _dev(y), _net(kind), return_maps=True, return_features=True, return_tap_values=True)
    torch.cuda.synchronize()
    tag = "%dx%d %s" % (h, w, kind)
    sides = lp.level_sides(h, w)
    assert tuple(value.shape) == (1,) and value.dtype == torch.float32 and tuple(taps.shape) == (1, 5)
    for k in range(5):
        assert tuple(fx[k].shape) == tuple(fy[k].shape) == (ref.TAP_CHANNELS[k],) + sides[k] and tuple(maps[k].shape) == (1,) + sides[k], (tag, k)
    got = {}
    for k in range(5):
        got["tap%d x" % (k + 1)], got["tap%d y" % (k + 1)], got["map%d" % (k + 1)] = fx[k], fy[k], maps[k][0]
    failed = []
    for name, arr in ref.flat_items(want):          # everything is printed before the first failure is raised: the first item off its bar localises it
        try:
            _check("%s %s" % (tag, name), got[name], arr, d_ref[name], both[name])
        except AssertionError as e:
            failed.append(e)
    if failed:
        raise failed[0]
    # the scalar: within the maps' yardsticks of the arbiter, and exactly the float64 sum of the float64 means of the returned maps, rounded once
    bound = F64_K * sum(d_ref["map%d" % (k + 1)] for k in range(5))
    err = abs(float(value[0]) - float(want["lpips"]))
    print("%-28s lpips %.9f  f64 %.9f  err %.3e  bound %.3e" % (tag, float(value[0]), float(want["lpips"]), err, bound))
    assert np.isfinite(float(value[0])) and err <= bound, (tag, err, bound)
    means = [m[0].double().cpu().numpy().mean(dtype=np.float64) for m in maps]
    assert float(value[0]) == float(np.float32(np.sum(np.array(means, dtype=np.float64)))), tag
    assert taps[0].tolist() == [float(np.float32(m)) for m in means], tag
    return value, maps, fx, fy, taps


# ---- 1. frames against the bar -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", FRAMES)
def test_taps_maps_and_scalar_against_float64(h, w):
    value, maps, fx, fy, taps = _parity(h, w, "default")
    assert 0.005 < float(value[0]) < 0.2          # y = clamp(x + 0.1 randn): a small, non-zero distance
    for k in range(5):
        dead = float((fx[k] == 0).float().mean())
        assert 0.3 < dead < 0.7, (k, dead)          # about half of every tap is ReLU-dead: a skipped store would hide behind a stale zero there


def test_dead_tap5():
    h, w = 33, 37
    value, maps, fx, fy, taps = _parity(h, w, "dead_tap5")
    assert not bool(fx[4].any()) and not bool(fy[4].any()) and not bool(maps[4].any())          # exactly zero: 0 / (0 + 1e-10), not NaN
    assert float(taps[0, 4]) == 0.0 and bool((taps[0, :4] > 0).all())
    assert bool(torch.isfinite(value).all()) and all(bool(torch.isfinite(m).all()) for m in maps)


# ---- 2. exact properties -------------------------------------------------------------------------------------------------------------------------------
def test_exact_properties():
    net = _net()
    x, y = (_dev(a) for a in _pair(17, 19))
    x2, y2 = (_dev(a) for a in _pair(17, 19)[::-1])
    g = torch.Generator(device="cpu").manual_seed(3)
    z = torch.rand((3, 17, 19), generator=g).cuda()
    base = lp.lpips(x, y, net)
    # identity and symmetry
    same, same_maps = lp.lpips(x, x, net, return_maps=True)
    assert torch.equal(same, torch.zeros_like(same)) and all(not bool(m.any()) for m in same_maps)
    assert torch.equal(lp.lpips(y, x, net), base) and torch.equal(lp.lpips(x2, y2, net), base)
    # a pair of a batch of 3 with mixed content equals that pair alone
    rs, gs = torch.stack([x, z, y]), torch.stack([y, x, z])
    batch, batch_maps = lp.lpips(rs, gs, net, return_maps=True)
    assert tuple(batch.shape) == (3,) and len(set(batch.tolist())) == 3
    for i in range(3):
        alone, alone_maps = lp.lpips(rs[i], gs[i], net, return_maps=True)
        assert torch.equal(alone[0], batch[i]) and all(torch.equal(a[0], b[i]) for a, b in zip(alone_maps, batch_maps)), i
    # two calls on two streams give the same bits
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            outs.append(lp.lpips(x, y, net, return_maps=True))
        s.synchronize()
    assert torch.equal(outs[0][0], base) and torch.equal(outs[1][0], base) and all(torch.equal(a, b) for a, b in zip(outs[0][1], outs[1][1]))
    # non-contiguous and channel-last inputs give the bits of their contiguous copies
    wide = torch.rand((3, 17, 40), generator=g).cuda()
    strided = wide[:, :, ::2][:, :, :19]
    assert not strided.is_contiguous()
    assert torch.equal(lp.lpips(strided, y, net), lp.lpips(strided.contiguous(), y, net))
    last = rs.contiguous(memory_format=torch.channels_last)
    assert not last.is_contiguous() and torch.equal(lp.lpips(last, gs, net), batch)
    hwc = x.permute(1, 2, 0).contiguous().permute(2, 0, 1)
    assert not hwc.is_contiguous() and torch.equal(lp.lpips(hwc, y, net), base)
    # other floating dtypes are converted, and the module's forward is the function
    assert torch.equal(lp.lpips(x.double(), y.double(), net), base) and torch.equal(net(x, y), base)


# ---- 3. loading ----------------------------------------------------------------------------------------------------------------------------------------
def test_state_dict_namings_give_the_same_bits():
    own, tv, theirs = ref.state_dicts(_params("default"))
    assert any(k.startswith("classifier.") for k in tv) and "net.mean" in theirs
    x, y = (_dev(a) for a in _pair(16, 16))
    base = lp.lpips(x, y, _net(), return_maps=True)
    for sd in (own, tv, theirs):
        net = lp.LPIPSNet()
        result = net.load_state_dict(dict(sd))
        assert not result.missing_keys and not result.unexpected_keys
        assert all(not p.requires_grad for p in net.parameters()) and len(list(net.parameters())) == 31
        got = lp.lpips(x, y, net.cuda(), return_maps=True)
        assert torch.equal(got[0], base[0]) and all(torch.equal(a, b) for a, b in zip(got[1], base[1]))
    # a freshly constructed network has other (random) values of the same shapes
    fresh = lp.LPIPSNet()
    assert {k: tuple(v.shape) for k, v in fresh.state_dict().items()} == {k: tuple(v.shape) for k, v in own.items()}
    assert not torch.equal(lp.lpips(x, y, fresh.cuda()), base[0])


def test_named_refusals():
    own, tv, theirs = ref.state_dicts(_params("default"))
    twice = dict(tv)
    twice["conv3_2_w"] = own["conv3_2_w"]
    with pytest.raises(ValueError, match=r"conv3_2_w.*given twice"):
        lp.LPIPSNet().load_state_dict(twice)
    twice = dict(own)
    twice["lin.2.1.weight"] = theirs["lin.2.1.weight"]
    with pytest.raises(ValueError, match=r"lin3_w.*given twice"):
        lp.LPIPSNet().load_state_dict(twice)
    bad = dict(theirs)
    bad["net.layers.17.weight"] = torch.zeros(512, 256, 1, 1)
    with pytest.raises(ValueError, match=r"wrong shape.*conv4_1_w"):
        lp.LPIPSNet().load_state_dict(bad)
    bad = dict(tv)
    bad["lin4.model.1.weight"] = torch.zeros(1, 256, 1, 1)
    with pytest.raises(ValueError, match=r"wrong shape.*lin5_w"):
        lp.LPIPSNet().load_state_dict(bad)
    missing = dict(tv)
    del missing["features.28.bias"]
    with pytest.raises(KeyError, match=r"missing layer.*conv5_3_b"):
        lp.LPIPSNet().load_state_dict(missing)
    net = _net()
    x = torch.rand(3, 16, 16).cuda()
    with pytest.raises(RuntimeError, match="MI355X only"):
        lp.lpips(x, x.cpu(), net)
    with pytest.raises(RuntimeError, match="MI355X only"):
        lp.lpips(x, x, lp.LPIPSNet())
    for shape in ((4, 16, 16), (2, 1, 16, 16)):
        with pytest.raises(ValueError, match="channels"):
            lp.lpips(torch.rand(shape).cuda(), torch.rand(shape).cuda(), net)
    for shape in ((3, 15, 16), (3, 16, 15), (1, 3, 16, 4097)):
        with pytest.raises(ValueError, match="out of range"):
            lp.lpips(torch.empty(shape, device="cuda"), torch.empty(shape, device="cuda"), net)


# ---- 4. image_eval -------------------------------------------------------------------------------------------------------------------------------------
def test_image_eval_carries_lpips():
    net = _net()
    views = [(16, 16), (17, 19), (16, 16)]
    g = torch.Generator(device="cpu").manual_seed(7)
    renders = [torch.rand((3, h, w), generator=g).cuda() for h, w in views]
    gts = [(r + 0.05 * torch.rand(r.shape, generator=g).cuda()).clamp(0, 1) for r in renders]
    names = ["a", "b", "c"]
    plain = image_eval.evaluate_images(renders, gts, names)
    assert sorted(plain) == ["PSNR", "SSIM", "per_view"] and sorted(plain["per_view"]) == ["PSNR", "SSIM"]
    full = image_eval.evaluate_images(renders, gts, names, lpips_net=net)
    assert sorted(full) == ["LPIPS", "PSNR", "SSIM", "per_view"] and sorted(full["per_view"]) == ["LPIPS", "PSNR", "SSIM"]
    assert full["SSIM"] == plain["SSIM"] and full["PSNR"] == plain["PSNR"]
    assert full["per_view"]["SSIM"] == plain["per_view"]["SSIM"] and full["per_view"]["PSNR"] == plain["per_view"]["PSNR"]
    each = [float(lp.lpips(r, t, net)[0]) for r, t in zip(renders, gts)]
    assert [full["per_view"]["LPIPS"][n] for n in names] == each and len(set(each)) == 3
    assert full["LPIPS"] == pytest.approx(sum(each) / 3, rel=1e-6)
    m_plain = image_eval.image_metrics(renders[1], gts[1])
    m_full = image_eval.image_metrics(renders[1], gts[1], lpips_net=net)
    assert sorted(m_plain) == ["l1", "psnr", "ssim"] and sorted(m_full) == ["l1", "lpips", "psnr", "ssim"]
    assert all(torch.equal(m_plain[k], m_full[k]) for k in m_plain) and float(m_full["lpips"][0]) == each[1]


# ---- 5. dirty, guard-banded buffers (tests/dirty_alloc.py) -------------------------------------------------------------------------
def test_dirty_buffers():
    """The scalar, the tap values, the five maps and the arena may hold anything on entry; nothing outside them is written; the bits equal the plain run.  The
    taps are returned too: views into the arena, every element of which a launch of this call must have stored."""
    net = _net()
    x, y = (_dev(a) for a in _pair(17, 19))

    def call():
        # lpips, tap values, five maps, the arena (8)
        return lp.lpips(x, y, net, return_maps=True, return_features=True, return_tap_values=True)
    base = dict(da.check("lpips 17x19", call, "cuda", 1 + 1 + 5 + 1))
    assert len(base) == 1 + 5 + 10 + 1
    want, d_ref, both = _cpu(17, 19, "default")
    assert abs(float(base["[0]"][0]) - float(want["lpips"])) <= F64_K * sum(d_ref["map%d" % (k + 1)] for k in range(5))
