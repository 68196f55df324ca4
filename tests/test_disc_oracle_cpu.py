"""The float64 oracle of the K5 kernels (oracle/disc_ref.py) and the comparator of the GPU checks (tests/disc_compare.py), on the
CPU: the direct and expanded oracles are oracle/ref_cpu.disc_loss and its autograd in float64; the split oracle stays within the
bf16 bounds the older tests allow against the direct form; the oracle against itself, its inputs moved by one f32 ulp, stays under
the constants; and with those constants the comparator rejects every deliberately wrong variant in oracle/disc_ref.py's `_fault`
list.  None of the listed faults falls below the floor."""
import pytest
import torch

import disc_compare as DC
from oracle import ref_cpu as R
from oracle.disc_ref import disc_ref_bwd, disc_ref_fwd

C = 2.0  # hip_binding.INV_TWO_VAR: 1 / (2 exp(log 0.25))
D = 32


def _autograd(q, t, idx, gmul):
    """CE and its gradients through ref_cpu.disc_loss in float64, scaled by the f32 upstream gradient the kernels take."""
    qd, td = q.double().requires_grad_(True), t.double().requires_grad_(True)
    ce = R.disc_loss(qd, td, idx)
    ce.backward()
    g = torch.tensor(gmul, dtype=torch.float32).item() * q.shape[0]
    return ce.detach(), qd.grad * g, td.grad * g


@pytest.mark.parametrize("mode", ["direct", "expanded"])
@pytest.mark.parametrize("B,S,regime,pattern,row_chunk", [(300, 700, "unrelated", "edges", 1 << 25), (64, 129, "separated", "random", 1000),
                                                          (257, 33, "exact", "shared", 1 << 25), (40, 1, "unrelated", "random", 7)])
def test_unrounded_oracle_is_disc_loss_f64(mode, B, S, regime, pattern, row_chunk):
    q, t, idx = DC.make_inputs(B, S, D, regime, pattern, B + S)
    ce, dq, dt = _autograd(q, t, idx, 1.0 / B)
    f = disc_ref_fwd(q, t, idx, C, mode, max_elems=row_chunk)
    b = disc_ref_bwd(q, t, idx, C, f["rmax"], f["rsum"], 1.0, 1.0 / B, mode, max_elems=row_chunk)
    assert abs(f["ce"].item() - ce.item()) <= 1e-10 * max(1.0, abs(ce.item()))
    for got, want in ((b["dq"], dq), (b["dt"], dt)):
        assert (got - want).abs().max().item() <= 1e-10 * max(1e-30, want.abs().max().item())


def test_row_shards_combine_to_the_whole():
    """Three shards (row0 > 0 for two): the merged (max, sumexp, target) is the whole table's, and the shards' backwards with the
    merged statistics add up to the whole backward."""
    B, S = 300, 1000
    q, t, idx = DC.make_inputs(B, S, D, "unrelated", "edges", 3)
    for mode in DC.CONSTS:
        whole = disc_ref_fwd(q, t, idx, C, mode)
        cuts = [0, 333, 334, S]
        parts = [disc_ref_fwd(q, t[a:b], idx, C, mode, row0=a) for a, b in zip(cuts[:-1], cuts[1:])]
        lse = torch.logsumexp(torch.stack([p["lse"] for p in parts]), 0)
        tgt = sum(p["tgt"] for p in parts)
        assert (lse - whole["lse"]).abs().max().item() < 1e-10 and (tgt - whole["tgt"]).abs().max().item() < 1e-12
        wb = disc_ref_bwd(q, t, idx, C, whole["rmax"], whole["rsum"], 0.7, 1.0 / B, mode)
        dq = torch.zeros_like(wb["dq"])
        for a, b in zip(cuts[:-1], cuts[1:]):
            sb = disc_ref_bwd(q, t[a:b], idx, C, whole["rmax"], whole["rsum"], 0.7, 1.0 / B, mode, row0=a)
            dq += sb["dq"]
            assert (sb["dt"] - wb["dt"][a:b]).abs().max().item() <= 1e-12 * wb["dt"].abs().max().item()
        assert (dq - wb["dq"]).abs().max().item() <= 1e-12 * wb["dq"].abs().max().item()


@pytest.mark.parametrize("regime,noise", [("unrelated", None), ("converged", 0.05)])
def test_split_oracle_within_the_bf16_bounds_of_the_direct_form(regime, noise):
    """The rounding model is not off by more than the bf16 mode is allowed today (test_config_parity_gpu._disc_bf16_case): CE
    within 2e-3 relative + 4x the 2^-16 logit resolution, each gradient within 1e-2 of its max + the same floor."""
    B, S = 300, 5000
    torch.manual_seed(B + S + 1)
    t = torch.randn(S, D)
    idx = torch.randint(0, S, (B,))
    q = torch.randn(B, D) if noise is None else t[idx] + noise * torch.randn(B, D)
    ce, dq, dt = _autograd(q, t, idx, 1.0 / B)
    f = disc_ref_fwd(q, t, idx, C, "split")
    b = disc_ref_bwd(q, t, idx, C, f["rmax"], f["rsum"], 1.0, 1.0 / B, "split", tgt=f["tgt"].float())
    resolution = 2.0 ** -16 * 2 * C * (D * 2)
    assert abs(f["ce"].item() - ce.item()) <= 2e-3 * abs(ce.item()) + 4 * resolution
    spread = (2 * noise * D ** 0.5) if noise is not None else (2 * D ** 0.5)
    g_floor = 4 * resolution * 2 * C * spread / B + 1e-9
    for got, want in ((b["dq"], dq), (b["dt"], dt)):
        assert (got - want).abs().max().item() <= 1e-2 * want.abs().max().item() + g_floor


def _ulp(x, g):
    """x with a random half of its entries moved one f32 ulp up or down."""
    up = torch.nextafter(x, torch.full_like(x, float("inf")))
    dn = torch.nextafter(x, torch.full_like(x, -float("inf")))
    y = torch.where(torch.rand(x.shape, generator=g) < 0.5, up, dn)
    return torch.where(torch.rand(x.shape, generator=g) < 0.5, y, x)


def _as_kernel(f):
    """The forward as a kernel leaves it: f32 statistics and target logits."""
    return {"rmax": f["rmax"].float(), "rsum": f["rsum"].float(), "tgt": f["tgt"].float(), "ce": f["ce"].float().item()}


GS = 0.7


def _judge(mode, consts, q, t, idx, got_mode=None, fault=None, base=None, quiet=True, label=""):
    """Failures of the oracle of `got_mode` (with `fault`, inputs `base` = (q, t) or q, t) against the oracle of `mode`, with the
    constants `consts`; the backward of both from the 'kernel's' statistics, upstream gradient GS * (-1/B)."""
    got_mode = got_mode or mode
    B = q.shape[0]
    gm = -1.0 / B
    qg, tg = base if base is not None else (q, t)
    fg = _as_kernel(disc_ref_fwd(qg, tg, idx, C, got_mode, _fault=fault))
    fw = disc_ref_fwd(q, t, idx, C, mode)
    bg = disc_ref_bwd(qg, tg, idx, C, fg["rmax"], fg["rsum"], GS, gm, got_mode, tgt=fg["tgt"], _fault=fault)
    bw = disc_ref_bwd(q, t, idx, C, fg["rmax"], fg["rsum"], GS, gm, mode, tgt=fg["tgt"])
    bg = {k: v.float() for k, v in bg.items()}
    bad = DC.compare_fwd(fg, fw, q, t, idx, C, consts, label, quiet)
    return bad + DC.compare_bwd(bg, bw, q, t, C, GS * gm, consts, label, quiet)


@pytest.mark.parametrize("B,S", [(300, 4633), (1000, 9000)])
@pytest.mark.parametrize("mode", list(DC.CONSTS))
def test_floor_is_below_the_constants(mode, B, S):
    """The oracle against itself, q and the table moved by one f32 ulp (the split operands kept: see oracle/disc_ref.py), passes
    with the constants the GPU file uses; the numbers are in tests/disc_compare.py."""
    bad = []
    for regime in DC.REGIMES:
        for pattern in ("random", "edges"):
            q, t, idx = DC.make_inputs(B, S, D, regime, pattern, 7)
            g = torch.Generator().manual_seed(3)
            fault = {"split_from": (q, t)} if mode == "split" else None
            bad += _judge(mode, DC.CONSTS[mode], q, t, idx, fault=fault, base=(_ulp(q, g), _ulp(t, g)),
                          quiet=False, label="%s %s %s" % (mode, regime, pattern))
    assert not bad, bad


# each fault, with the form it belongs to; checked on two regimes (q unrelated to the table; separated: where the own row carries
# the softmax for half the queries), ragged B = 300 (44 queries in the last tile) and S = 4633 (a 25-row last table tile)
FAULTS = [("split", {"no_qlo_thi": True}), ("split", {"W_unrounded": True}), ("split", {"G_no_ylo": True}),
          ("expanded", {"own_twice": True}), ("split", {"own_twice": True}),
          ("expanded", {"own_grad_dropped": True}), ("split", {"own_grad_dropped": True}),
          ("expanded", {"drop_tail_tile": True}), ("split", {"drop_tail_tile": True}), ("direct", {"drop_tail_tile": True}),
          ("expanded", {"drop_queries": 16}), ("split", {"drop_queries": 16}), ("direct", {"drop_queries": 16})]


@pytest.mark.parametrize("mode,fault", FAULTS, ids=["%s-%s" % (m, next(iter(f))) for m, f in FAULTS])
def test_comparator_rejects_fault(mode, fault):
    B, S = 300, 4633
    bad = {}
    for regime in ("unrelated", "separated"):
        q, t, idx = DC.make_inputs(B, S, D, regime, "edges", 11)
        bad[regime] = _judge(mode, DC.CONSTS[mode], q, t, idx, fault=fault, quiet=False, label="%s %s" % (regime, fault))
    assert bad["unrelated"] or bad["separated"], "fault %s not seen" % fault


@pytest.mark.parametrize("got,want", [("expanded", "split"), ("split", "expanded")])
def test_comparator_tells_the_forms_apart(got, want):
    """A kernel that silently ran the other matrix-core form fails against its own form's oracle and constants."""
    q, t, idx = DC.make_inputs(300, 4633, D, "unrelated", "random", 5)
    assert _judge(want, DC.CONSTS[want], q, t, idx, got_mode=got, quiet=False, label="%s as %s" % (got, want))
