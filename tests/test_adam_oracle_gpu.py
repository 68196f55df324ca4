"""The fused Adam step (hip_binding.adam_step_ -> fhvae_adam_step, csrc/loss.hip:384-458; hip_optim.FusedAdam) against the float64
oracle of its own arithmetic (oracle/adam_ref.py) with the one comparator and the derived bounds of tests/adam_compare.py.

Every comparison is one step from the device's own state (p, g, m, v copied to the CPU before the launch), no element left out.
The cases reach every path of the kernel: the float4 loop, its n % 4 tail, the scalar loop taken when any of p, g, m, v is not
16-byte aligned, the second iteration of the grid-stride loop (n just over 8192 x 256 x 4), the bf16 shadow stores of all three
loops, grad_scale != 1, step counts 1 ... 100000 and the two-level step counter at 1, 2, 63, 64, 65, 66, 128, 129, 130 and 8192
workgroups.  Each case prints the worst error / bound ratio of p, m, v and the update.

Measured on an MI355X, the worst ratio over every case: p 0.995 (the store's rounding: u |p| is exactly half an ulp where the
mantissa is 1.0, so large cases come close by construction), m 0.57, v 0.63, the update 0.16 (its bound is mostly the allowance
for the f32 bias corrections, which the device's powf barely uses); FusedAdam's 30-step movement 0.12 of the summed bound.
"""
import pytest
import torch

import adam_compare as AC
from oracle.adam_ref import f32

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS = 3e-4, 0.95, 0.999, 1e-6  # lr and eps distinct from each other and from the defaults: a swapped argument shows
BETAS = [(0.95, 0.999), (0.9, 0.99), (0.0, 0.999)]
STEPS = [1, 2, 3, 10, 1000, 100000]
SCALES = [1.0, 1.0 / 8, 1.0 / 3]
HYPER = [(3e-4, 1e-6), (1e-3, 1e-8)]
WG = 4 * 256  # elements per workgroup
SIZES = [1, 2, 3, 4, 5, 7, 1023, 1024, 1027, WG * 63, WG * 64 + 1, WG * 65 + 2, WG * 129 + 3]
BIG = AC.GRID_CAP_ELEMS + 1029  # some lanes take a second iteration of the grid-stride loop, and a tail remains
FILL = 7.0


@pytest.fixture(scope="module")
def hb():
    import build_ext

    build_ext.build(verbose=False)
    import hip_binding

    hip_binding.load_library()
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return hip_binding


class Dev:
    """A case on the device.  Each of p, g, m, v is a view `lead` elements into a 16-byte aligned buffer filled with FILL, `trail`
    fill elements behind it (lead = 1: the view is 4 bytes off, the kernel's scalar path; lead = 4: aligned, padded)."""

    def __init__(self, case, leads=(0, 0, 0, 0), trail=0):
        self.n = case["p"].numel()
        self.buf, self.view, self.span = {}, {}, {}
        for k, lead in zip("pgmv", leads):
            b = torch.full((lead + self.n + trail,), FILL, device="cuda")
            assert b.data_ptr() % 16 == 0
            self.buf[k], self.span[k] = b, (lead, lead + self.n)
            self.view[k] = b[lead:lead + self.n]
            self.view[k].copy_(case[k])

    def pads_intact(self):
        return all(bool((b[:self.span[k][0]] == FILL).all()) and bool((b[self.span[k][1]:] == FILL).all()) for k, b in self.buf.items())


def _shadow(n, lead=0, trail=0):
    """A bf16 p_lp view `lead` elements (2 bytes each) into a buffer of FILL."""
    b = torch.full((lead + n + trail,), FILL, device="cuda", dtype=torch.bfloat16)
    return b, b[lead:lead + n]


def _shadow_ok(buf, view, p, lead):
    """p_lp is the new f32 p rounded to bf16, bit for bit, and nothing outside the view was written."""
    n = view.numel()
    return (torch.equal(view.view(torch.int16), p.bfloat16().view(torch.int16)) and bool((buf[:lead] == FILL).all())
            and bool((buf[lead + n:] == FILL).all()))


def _step_buf(hb, count):
    s = torch.zeros(hb.ADAM_STEP_WORDS, dtype=torch.int32, device="cuda")
    s[0] = count
    return s


def _launch(hb, d, t, lr=LR, b1=B1, b2=B2, eps=EPS, s=1.0, flags=0, p_lp=None, v_abs=None, step=None):
    """One launch at step count t (written into the step word; with ADAM_ADVANCE the word holds t - 1) and its comparison with the
    oracle's step from the state the launch found.  Returns (ratios, that state, the step buffer)."""
    before = {k: d.view[k].cpu() for k in "pgmv"}
    if step is None:
        step = _step_buf(hb, t - 1 if flags & hb.ADAM_ADVANCE else t)
    hb.adam_step_(d.view["p"], d.view["g"], d.view["m"], d.view["v"], step, lr, b1, b2, eps, s, p_lp, flags)
    torch.cuda.synchronize()
    return AC.compare(before, d.view, t, lr, b1, b2, eps, s, v_abs), before, step


@pytest.mark.parametrize("n", SIZES)
def test_sizes(hb, n):
    """n < 4, every tail length, one workgroup and the 64-group boundaries: the float4 loop and its tail, with the bf16 shadow."""
    d = Dev(AC.make_case(n, n, B1, B2))
    buf, lp = _shadow(n)
    r, before, step = _launch(hb, d, 3, p_lp=lp)
    AC.check(r, "size %d" % n)
    assert _shadow_ok(buf, lp, d.view["p"], 0)
    assert torch.equal(d.view["g"].cpu(), before["g"])  # without ZERO_GRAD g is bit-identical
    assert step.tolist() == [3] + [0] * (hb.ADAM_STEP_WORDS - 1)  # without ADVANCE the step buffer is only read


@pytest.mark.parametrize("which", ["all", "p", "g", "m", "v"])
@pytest.mark.parametrize("n", [5, 1027, WG * 65 + 2])
def test_scalar_path(hb, n, which):
    """All four arrays, then each alone, 4 bytes off 16-byte alignment: the scalar loop.  p_lp sits 2 bytes into its buffer; with
    ZERO_GRAD every element of g is cleared, and nothing outside any view is written."""
    leads = tuple(1 if which in ("all", k) else 0 for k in "pgmv")
    d = Dev(AC.make_case(n, n + 11, B1, B2, 1.0 / 8), leads, trail=3)
    assert any(d.view[k].data_ptr() % 16 for k in "pgmv")
    buf, lp = _shadow(n, 1, 5)
    r, before, _ = _launch(hb, d, 2, s=1.0 / 8, flags=hb.ADAM_ZERO_GRAD, p_lp=lp)
    AC.check(r, "scalar path (%s off) n %d" % (which, n))
    assert _shadow_ok(buf, lp, d.view["p"], 1)
    assert not d.view["g"].any() and d.pads_intact()


@pytest.mark.parametrize("lead", [4, 1])
def test_padded_views(hb, lead):
    """Views with padding on both sides (aligned: the float4 loop and a 3-element tail; one element off: the scalar loop): the pad
    elements of p, g, m, v and p_lp keep their fill value."""
    n = 1027
    d = Dev(AC.make_case(n, 77 + lead, B1, B2), (lead,) * 4, trail=9)
    buf, lp = _shadow(n, 8, 8)
    r, _, step = _launch(hb, d, 10, flags=hb.ADAM_ZERO_GRAD | hb.ADAM_ADVANCE, p_lp=lp)
    AC.check(r, "padded views, lead %d" % lead)
    assert d.pads_intact() and _shadow_ok(buf, lp, d.view["p"], 8)
    assert not d.view["g"].any() and step.tolist() == [10] + [0] * (hb.ADAM_STEP_WORDS - 1)


def test_hyper_parameters_and_step_counts(hb):
    """Every beta pair x step count x gradient scale at n = 1027, lr and eps alternating between two distinct pairs.  At
    t = 100000 the first correction is exactly 1; b1 = 0 makes m the scaled gradient."""
    n, worst = 1027, dict.fromkeys(AC.KEYS, 0.0)
    for bi, (b1, b2) in enumerate(BETAS):
        for ti, t in enumerate(STEPS):
            for si, s in enumerate(SCALES):
                lr, eps = HYPER[(bi + ti + si) % 2]
                d = Dev(AC.make_case(n, 100 * bi + 10 * ti + si, b1, b2, s))
                r, _, _ = _launch(hb, d, t, lr, b1, b2, eps, s)
                AC.check(r, "b (%g, %g) s %.3g lr %g eps %g" % (b1, b2, s, lr, eps))
                worst = {k: max(worst[k], r[k]) for k in AC.KEYS}
    print("adam grid, worst ratios: %s" % "  ".join("%s %.3f" % kv for kv in worst.items()))


def test_zero_state_first_step(hb):
    d = Dev(AC.make_case(1027, 21, B1, B2, warm=0))
    assert not d.view["m"].any() and not d.view["v"].any()
    AC.check(_launch(hb, d, 1, flags=hb.ADAM_ADVANCE)[0], "zero state, t 1")


def test_gradients_whose_square_underflows(hb):
    """|g| in [1e-30, 1e-20]: gi^2 underflows, sqrt(v_hat) is far below eps.  Finite, p, m and the update within their bounds, v
    within 2^-126 absolute."""
    d = Dev(AC.make_case(1027, 22, B1, B2, kind="tiny"))
    r = _launch(hb, d, 3, eps=1e-8, v_abs=AC.V_TINY)[0]
    assert r["finite"]
    AC.check(r, "tiny gradients")


def test_zero_gradient_from_zero_state_moves_nothing(hb):
    case = AC.make_case(1027, 23, B1, B2, kind="zero", warm=0)
    d = Dev(case)
    r = _launch(hb, d, 1, eps=1e-8, flags=hb.ADAM_ADVANCE)[0]
    AC.check(r, "zero gradient, zero state")
    assert torch.equal(d.view["p"].cpu().view(torch.int32), case["p"].view(torch.int32))  # bit-identical
    assert not d.view["m"].any() and not d.view["v"].any()
    assert all(bool(torch.isfinite(d.view[k]).all()) for k in "pmv")


@pytest.mark.parametrize("n", [1, 1027, WG * 63, WG * 64, WG * 64 + 1, WG * 65 + 2, WG * 128, WG * 129, WG * 129 + 3, BIG])
def test_flags_over_three_launches(hb, n):
    """ADAM_ADVANCE at 1, 2, 63, 64, 65, 66, 128, 129, 130 workgroups and at the capped grid (8192, with a second grid-stride
    iteration): step[0] counts 1, 2, 3, every other word of the step buffer is 0 after every launch, and each launch passes at its
    own t.  The first launch also has ADAM_ZERO_GRAD (g all zero afterwards); the others leave g bit-identical."""
    s = 1.0 / 8
    case = AC.make_case(n, n % 1009, B1, B2, s, warm=1 if n == BIG else 3)
    d = Dev(case)
    step = _step_buf(hb, 0)
    for k in range(3):
        flags = hb.ADAM_ADVANCE | (hb.ADAM_ZERO_GRAD if k == 0 else 0)
        if k:
            d.view["g"].copy_(case["g"].roll(k))
        r, before, _ = _launch(hb, d, k + 1, s=s, flags=flags, step=step)
        AC.check(r, "flags n %d launch %d" % (n, k + 1))
        assert step.tolist() == [k + 1] + [0] * (hb.ADAM_STEP_WORDS - 1)
        if k == 0:
            assert not d.view["g"].any()
        else:
            assert torch.equal(d.view["g"].cpu(), before["g"])


def test_operands_are_checked_before_the_launch(hb):
    """A g, m or v of another length, a dtype other than float32, a non-contiguous view, a p_lp that is not bf16 of n contiguous
    elements: RuntimeError, and nothing is written."""
    n = 64
    good = {k: torch.full((n,), 1.0 + i, device="cuda") for i, k in enumerate("pgmv")}
    lp = torch.full((n,), FILL, device="cuda", dtype=torch.bfloat16)
    step = _step_buf(hb, 4)
    wide = torch.full((2 * n,), 5.0, device="cuda")
    bad = []
    for k in "gmv":
        bad.append({k: torch.full((n - 1,), 9.0, device="cuda")})
        bad.append({k: torch.full((n + 1,), 9.0, device="cuda")})
    for k in "pgmv":
        bad.append({k: good[k].double()})
        bad.append({k: good[k].bfloat16()})
        bad.append({k: wide[::2]})
    bad += [{"p_lp": torch.zeros(n, device="cuda")}, {"p_lp": torch.zeros(n, device="cuda", dtype=torch.float16)},
            {"p_lp": lp[:n - 1]}, {"p_lp": torch.zeros(2 * n, device="cuda", dtype=torch.bfloat16)[::2]},
            {"p": good["p"][:n - 1]}]
    for sub in bad:
        a = dict(good, p_lp=lp)
        a.update(sub)
        keep = {k: v.clone() for k, v in a.items()}
        with pytest.raises(RuntimeError):
            hb.adam_step_(a["p"], a["g"], a["m"], a["v"], step, LR, B1, B2, EPS, 1.0, a["p_lp"], hb.ADAM_ZERO_GRAD | hb.ADAM_ADVANCE)
        torch.cuda.synchronize()
        assert all(torch.equal(a[k], keep[k]) for k in a), sorted(sub)
        assert bool((wide == 5.0).all()) and step.tolist() == [4] + [0] * (hb.ADAM_STEP_WORDS - 1)
    # ... and the well-formed call goes through
    hb.adam_step_(good["p"], good["g"], good["m"], good["v"], step, LR, B1, B2, EPS, 1.0, lp, hb.ADAM_ZERO_GRAD | hb.ADAM_ADVANCE)
    assert int(step[0]) == 5 and not good["g"].any()


def test_fused_adam_thirty_steps_and_resume(hb):
    """hip_optim.FusedAdam over three parameters whose sizes are no multiples of 64, grad_scale = 1/4, 30 steps of mixed-magnitude
    gradients, against torch.optim.Adam in float64 on the CPU over g / 4 with the rounded hyper-parameters: the accumulated
    movement p_30 - p_0 of every element agrees to the sum of the per-step bounds along the oracle's trajectory; the arena's padding
    stays exactly 0; and after load_state_dict with step = 100000 the next step passes compare() at t = 100001."""
    from hip_optim import FusedAdam

    shapes, s, steps = [(7, 5), (13,), (33, 3)], 0.25, 30
    sizes = [int(torch.Size(sh).numel()) for sh in shapes]
    gen = torch.Generator().manual_seed(31)
    p0 = [AC.make_case(n, 40 + i, B1, B2, warm=0)["p"] for i, n in enumerate(sizes)]
    grads = [[AC.make_grad(n, gen, s, phase=k) for n in sizes] for k in range(steps)]
    mine = [torch.nn.Parameter(p.view(sh).clone().cuda()) for p, sh in zip(p0, shapes)]
    opt = FusedAdam(mine, lr=LR, betas=(B1, B2), eps=EPS, grad_scale=s)
    ref = [p.double().clone().requires_grad_(True) for p in p0]
    o_ref = torch.optim.Adam(ref, lr=f32(LR), betas=(f32(B1), f32(B2)), eps=f32(EPS))
    for gs in grads:
        with torch.no_grad():
            for prm, r, g in zip(mine, ref, gs):
                prm.grad.copy_(g.view(prm.shape))
                r.grad = g.double() * s
        opt.step()
        o_ref.step()
    torch.cuda.synchronize()
    assert int(opt.step_dev.item()) == steps and not opt.g_arena.flat.any()
    worst = 0.0
    for i, (prm, r, p) in enumerate(zip(mine, ref, p0)):
        po, _, _, total = AC.trajectory(p, [gs[i] for gs in grads], LR, B1, B2, EPS, s)
        assert ((po - r.detach()).abs() <= 1e-12 * po.abs()).all()
        moved_k = prm.detach().cpu().double().reshape(-1) - p.double()
        moved_o = r.detach() - p.double()
        ratio = AC.ratio((moved_k - moved_o).abs(), total)
        print("adam FusedAdam parameter %d (%d elements): worst accumulated error / summed bound %.3f" % (i, sizes[i], ratio.max().item()))
        worst = max(worst, ratio.max().item())
    assert worst <= 1.0
    pad = torch.ones(opt.p_arena.numel, dtype=torch.bool)
    for off, n in zip(opt.p_arena.offsets, sizes):
        pad[off:off + n] = False
    assert pad.any()
    for name, t in (("p", opt.p_arena.flat), ("g", opt.g_arena.flat), ("m", opt.m), ("v", opt.v)):
        assert not t.cpu()[pad].any(), "arena padding of %s" % name
    # resume at a large step count: the whole arena, padding included, through the comparator
    sd = opt.state_dict()
    for st in sd["state"].values():
        st["step"] = torch.tensor(100000.0)
    opt.load_state_dict(sd)
    with torch.no_grad():
        for prm, g in zip(mine, grads[0]):
            prm.grad.copy_(g.view(prm.shape))
    before = {"p": opt.p_arena.flat.cpu(), "g": opt.g_arena.flat.cpu(), "m": opt.m.cpu(), "v": opt.v.cpu()}
    opt.step()
    torch.cuda.synchronize()
    assert int(opt.step_dev.item()) == 100001
    AC.check(AC.compare(before, {"p": opt.p_arena.flat, "m": opt.m, "v": opt.v}, 100001, LR, B1, B2, EPS, s), "FusedAdam resumed at 100000")
    assert not opt.p_arena.flat.cpu()[pad].any()
