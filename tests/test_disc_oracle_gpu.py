"""Every form of K5 (hip_binding.raw_disc_fwd / raw_disc_bwd / disc_lse) against the float64 oracle of its own arithmetic
(oracle/disc_ref.py), with one comparator and one set of constants per form (tests/disc_compare.py): the VALU direct form
(disc.hip), the exact-f32 MFMA expanded form (disc_mfma.hip) and the bf16 split-operand form (disc_lp.hip), each MFMA form's
forward and its backward as two passes (ws_bytes = 0), one pass over the whole problem (MODE 2) and one pass in query groups of
one and of two 256-query tiles.  Each case prints its measurements and, for comparison, the same numbers against the exact direct
form.  The oracle runs in float64 on the GPU (torch's dgemm), the tensors never leave the device."""
import pytest
import torch

import disc_compare as DC
from disc_plan import cdiv as _cdiv, group_bytes as _group_bytes
from oracle.disc_ref import disc_ref_bwd, disc_ref_fwd

pytestmark = pytest.mark.gpu

GS = 0.7


@pytest.fixture(scope="module")
def hb():
    import build_ext

    build_ext.build(verbose=False)
    import hip_binding

    hip_binding.load_library()
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return hip_binding


def _form(B, S, D, lp):
    """The form fhvae_disc_lse_fwd / _bwd dispatch to (disc.hip disc_engine: direct = the VALU kernels, expanded = disc_mfma.hip, split = disc_lp.hip)."""
    if D in (16, 32) and B * S >= 65536:
        return "split" if lp and D == 32 else "expanded"
    return "direct"


def _sink(S, D, G0, seed):
    """A non-zero dt_sink (the kernels add into it): every 7th row G0 * 1e-3 * N(0,1), small enough that the f32 sum with the
    gradient rounds far below the floor."""
    g = torch.Generator().manual_seed(seed)
    s = torch.zeros(S, D)
    s[::7] = torch.randn(_cdiv(S, 7), D, generator=g) * G0 * 1e-3
    return s.cuda()


def _fwd_check(hb, q, t, idx, lp, form, label, row0=0):
    rmax, rsum, tgt, ce = hb.raw_disc_fwd(q, t, idx, row0=row0, lp=lp)
    got = {"rmax": rmax, "rsum": rsum, "tgt": tgt, "ce": ce.item()}
    want = disc_ref_fwd(q, t, idx, hb.INV_TWO_VAR, form, row0=row0)
    bad = DC.compare_fwd(got, want, q, t, idx, hb.INV_TWO_VAR, DC.CONSTS[form], label)
    if form != "direct":
        ex = disc_ref_fwd(q, t, idx, hb.INV_TWO_VAR, "direct", row0=row0)
        print("%s   (vs the direct form: %s)" % (label, DC.fmt_fwd(DC.measure_fwd(got, ex, DC.row_scale(q, t, hb.INV_TWO_VAR), idx))))
    return got, bad


def _bwd_variants(B, S, D, form):
    if form == "direct":
        return [("valu", None)]
    v = [("two-pass", 0), ("one-pass", None), ("groups1", _group_bytes(1, B, S, D))]
    if B > 512:
        v.append(("groups2", _group_bytes(2, B, S, D)))
    return v


def _bwd_check(hb, q, t, idx, lp, form, got_f, label, gmul, seed, row0=0, rmax=None, rsum=None, tgt=None):
    """Every backward variant of the form against one oracle backward (the kernel's own statistics)."""
    c = hb.INV_TWO_VAR
    B, D = q.shape
    S = t.shape[0]
    rmax = got_f["rmax"] if rmax is None else rmax
    rsum = got_f["rsum"] if rsum is None else rsum
    tgt = got_f["tgt"] if tgt is None else tgt
    want = disc_ref_bwd(q, t, idx, c, rmax, rsum, GS, gmul, form, row0=row0, tgt=tgt)
    ex = disc_ref_bwd(q, t, idx, c, rmax, rsum, GS, gmul, "direct", row0=row0, tgt=tgt) if form != "direct" else None
    G0 = DC.grad_scale(q, t, c, GS * gmul)
    gsc = torch.tensor([GS], device="cuda")
    bad = []
    for name, ws in _bwd_variants(B, S, D, form):
        sink0 = _sink(S, D, G0, seed)
        sink = sink0.clone()
        dq, _ = hb.raw_disc_bwd(q, t, idx, rmax, rsum, gsc, gmul, row0=row0, dt_sink=sink, lp=lp, ws_bytes=ws)
        got = {"dq": dq, "dt": sink.double() - sink0.double()}
        bad += DC.compare_bwd(got, want, q, t, c, GS * gmul, DC.CONSTS[form], "%s %s" % (label, name))
        if ex is not None:
            print("%s %s   (vs the direct form: dq %s | dt %s)" % (label, name, DC.fmt_grad(DC.measure_grad(dq, ex["dq"], G0, 1e-6, 256)),
                                                                 DC.fmt_grad(DC.measure_grad(got["dt"], ex["dt"], G0, 1e-6, 64))))
    return bad


def _case(hb, B, S, D, lp, regime, pattern, seed, gsign=1.0):
    q, t, idx = DC.make_inputs(B, S, D, regime, pattern, seed)
    q, t, idx = q.cuda(), t.cuda(), idx.cuda()
    form = _form(B, S, D, lp)
    label = "[%s B=%d S=%d D=%d %s %s]" % (form, B, S, D, regime, pattern)
    got_f, bad = _fwd_check(hb, q, t, idx, lp, form, label)
    bad += _bwd_check(hb, q, t, idx, lp, form, got_f, label, gsign / B, seed)
    return bad


# (B, S, D, regime, pattern): the configs' shapes, ragged and edge shapes; every MFMA case runs in both matrix-core forms
MFMA_CASES = [(2048, 28000, 32, "unrelated", "random"), (2048, 28000, 32, "converged", "edges"), (2048, 28000, 32, "separated", "shared"),
              (2048, 28000, 32, "exact", "random"),
              (256, 4600, 32, "unrelated", "edges"), (512, 100000, 32, "separated", "random"),
              (257, 4097, 32, "unrelated", "edges"), (300, 4633, 32, "separated", "edges"), (1000, 9000, 32, "unrelated", "shared"),
              (2048, 33, 32, "unrelated", "edges"), (65536, 1, 32, "unrelated", "random"), (256, 256, 32, "separated", "edges")]


@pytest.mark.parametrize("lp", [False, True], ids=["expanded", "split"])
@pytest.mark.parametrize("B,S,D,regime,pattern", MFMA_CASES)
def test_mfma_forms_against_their_oracle(hb, B, S, D, regime, pattern, lp):
    assert _form(B, S, D, lp) == ("split" if lp else "expanded")
    bad = _case(hb, B, S, D, lp, regime, pattern, B + S + int(lp), gsign=-1.0 if regime == "separated" else 1.0)
    assert not bad, bad


def test_split_form_at_the_rank_view(hb):
    """One rank's view of the largest config in bf16: 16384 queries x 12500 table rows."""
    bad = _case(hb, 16384, 12500, 32, True, "unrelated", "random", 5)
    assert not bad, bad


@pytest.mark.parametrize("B,S,D,lp", [(257, 255, 32, False), (257, 255, 32, True), (300, 4633, 8, True), (300, 4633, 64, False),
                                      (1000, 4097, 64, True)])
@pytest.mark.parametrize("regime,pattern", [("unrelated", "edges"), ("separated", "random")])
def test_valu_form_against_its_oracle(hb, B, S, D, lp, regime, pattern):
    """B * S = 65535 (one below the matrix-core threshold) and D = 8, 64: the VALU kernels in either compute mode."""
    assert _form(B, S, D, lp) == "direct"
    bad = _case(hb, B, S, D, lp, regime, pattern, B + S + D)
    assert not bad, bad


def test_d16_split_request_is_the_f32_form_bit_for_bit(hb):
    """D = 16 on the matrix cores: the bf16 mode has no split kernel there and must run the f32 one: its forward (no atomics) is
    the f32 forward bit for bit; the backward (atomics, so not bit-reproducible run to run) meets the expanded form's oracle."""
    B, S, D = 1000, 4633, 16
    q, t, idx = (x.cuda() for x in DC.make_inputs(B, S, D, "unrelated", "edges", 16))
    assert _form(B, S, D, True) == "expanded"
    a, b = hb.raw_disc_fwd(q, t, idx, lp=False), hb.raw_disc_fwd(q, t, idx, lp=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    bad = _case(hb, B, S, D, True, "unrelated", "edges", 16)
    assert not bad, bad


@pytest.mark.parametrize("lp", [False, True], ids=["expanded", "split"])
def test_row_shards(hb, lp):
    """Three shards of S = 28000 (row0 > 0 for two), targets inside and outside each: every shard's forward against the oracle of
    its rows, the merged statistics against the whole table's, each shard's backward with the merged global (rmax, rsum)."""
    B, S, D = 2048, 28000, 32
    c = hb.INV_TWO_VAR
    q, t, idx = (x.cuda() for x in DC.make_inputs(B, S, D, "unrelated", "edges", 28))
    form = "split" if lp else "expanded"
    cuts = [0, 9333, 18667, S]
    parts = torch.empty(3, 3, B, device="cuda")
    bad = []
    for w, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        ts = t[a:b].contiguous()
        inside = ((idx >= a) & (idx < b)).sum().item()
        assert 0 < inside < B
        hb.raw_disc_fwd(q, ts, idx, row0=a, want_ce=False, lp=lp, out3=parts[w])
        want = disc_ref_fwd(q, ts, idx, c, form, row0=a)
        bad += DC.compare_fwd({"rmax": parts[w, 0], "rsum": parts[w, 1], "tgt": parts[w, 2]}, want, q, ts, idx, c, DC.CONSTS[form],
                              "[%s shard %d row0=%d]" % (form, w, a))
    m, s, tg = hb.disc_merge_partials(parts)
    whole = disc_ref_fwd(q, t, idx, c, form)
    bad += DC.compare_fwd({"rmax": m, "rsum": s, "tgt": tg}, whole, q, t, idx, c, DC.CONSTS[form], "[%s merged]" % form)
    for w, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        ts = t[a:b].contiguous()
        bad += _bwd_check(hb, q, ts, idx, lp, form, None, "[%s shard %d bwd]" % (form, w), 1.0 / B, w, row0=a, rmax=m, rsum=s, tgt=tg)
    assert not bad, bad


@pytest.mark.parametrize("B,S,lp", [(2048, 28000, True), (2048, 28000, False), (300, 4633, True), (257, 255, True)])
def test_disc_lse_autograd_path(hb, B, S, lp):
    """hip_binding.disc_lse (the path the model takes): its CE and gradients against the oracle, upstream gradient 1 / B."""
    c = hb.INV_TWO_VAR
    D = 32
    q, t, idx = (x.cuda() for x in DC.make_inputs(B, S, D, "unrelated", "edges", B + S))
    form = _form(B, S, D, lp)
    qd, td = q.clone().requires_grad_(True), t.clone().requires_grad_(True)
    ce = hb.disc_lse(qd, td, idx, lp=lp)
    ce.backward()
    rmax, rsum, tgt, _ = hb.raw_disc_fwd(q, t, idx, lp=lp)  # (deterministic: the statistics the autograd forward saved)
    label = "[disc_lse %s B=%d S=%d]" % (form, B, S)
    want = disc_ref_fwd(q, t, idx, c, form)
    bad = DC.compare_fwd({"rmax": rmax, "rsum": rsum, "tgt": tgt, "ce": ce.item()}, want, q, t, idx, c, DC.CONSTS[form], label)
    wb = disc_ref_bwd(q, t, idx, c, rmax, rsum, 1.0, 1.0 / B, form, tgt=tgt)
    bad += DC.compare_bwd({"dq": qd.grad, "dt": td.grad}, wb, q, t, c, 1.0 / B, DC.CONSTS[form], label)
    assert not bad, bad
