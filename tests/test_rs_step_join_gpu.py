"""The join of the persistent recurrence kernels with one ticket line per XCD (csrc/lstm_cluster.h).  What fails without that layout
is the ticket-word check of test_repeated_backward_on_one_armed_block; every case also runs the join in front of a kernel and compares
the result with the rounding-faithful float64 oracle (oracle/lstm_lp_ref.py, standard comparator and constants of
tests/lstm_lp_compare.py).  Beyond the join, the other cases are extra coverage of the existing partial-dh backward
(csrc/lstm_bwd_rs.hip, unchanged) at the smallest shapes at which it runs (B = 1024 at H = 256): one exchange only (T = 2: step 0 has
no partials, the last step no product); first, middle and last step with dgsum and d_xc (T = 3, Ic > 0); a ragged last cluster
and a second launch of 6 rows (B = 1030: the rows past the end must leave the bias gradients and dgsum exact); d_hn without
d_hs_top and the reverse; the same backward three times on one armed sync block; and two contraction-split shapes."""
import pytest
import torch

from lstm_lp_compare import BF16, compare, make_inputs, named_tensors
from oracle.lstm_lp_ref import lstm_lp_ref

pytestmark = pytest.mark.gpu

RS, KS = 1, 2  # hb.LAST_LSTM_FORM["form"]: the rows form (H = 256: partial-dh backward), the contraction-split form
# word offsets of the sync block (csrc/lstm_cluster.h): the old ticket words, and one 128-byte line per XCD counter now
OLD_TICKETS, TICKETS, TICKET_STRIDE = 16, 2112, 32


@pytest.fixture(scope="module")
def hb():
    import build_ext

    build_ext.build(verbose=False)
    import hip_binding

    hip_binding.load_library()
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return hip_binding


_CACHE = {}


def _case(shape, partial_dh, use_out=True, use_hn=True):
    """Inputs and the oracle's tensors of one shape, computed once and shared (never modified)."""
    key = (shape, partial_dh, use_out, use_hn)
    if key not in _CACHE:
        B, T, I, Ic, H, L = shape
        x, xc, params, g_out, g_hn = make_inputs(B, T, I, Ic, H, L, B + 7 * T + H + L)
        if not use_hn:
            g_hn = torch.zeros_like(g_hn)
        ref = lstm_lp_ref(x, xc, params, g_out if use_out else None, g_hn, T=T, rounding=True,
                          **(dict(partial_dh_bf16=True) if partial_dh else {}))
        _CACHE[key] = (x, xc, params, g_out, g_hn, ref)
    return _CACHE[key]


def _forward(hb, x, xc, T, params, top):
    ps = [p.cuda().requires_grad_(True) for p in params]
    xcd = xc.cuda().requires_grad_(True) if xc is not None else None
    hs_top, hn = hb.lstm_seq(x.cuda() if x is not None else None, xcd, T, ps, hb.BF16, top=top)
    assert hb.LAST_LSTM_FORM["layout"] >= 16, hb.LAST_LSTM_FORM  # a persistent schedule
    return ps, xcd, hs_top, hn, hb.LAST_LSTM_FORM["form"]


def _check(hb, label, shape, form, top=2, use_out=True, use_hn=True):
    B, T, I, Ic, H, L = shape
    x, xc, params, g_out, g_hn, ref = _case(shape, form == RS, use_out and top != 0, use_hn)
    ps, xcd, hs_top, hn, got_form = _forward(hb, x, xc, T, params, top)
    assert got_form == form, (label, got_form)
    loss = None
    if use_hn:
        loss = (hn * g_hn.cuda()).sum()
    if use_out and top != 0:
        out = (hs_top * g_out.cuda()).sum()
        loss = out if loss is None else loss + out
    loss.backward()
    hb.flush_param_grads()
    torch.cuda.synchronize()
    assert hb.lstm_sync_status() == 0, "a persistent recurrence launch gave up"
    want = named_tensors(ref["hs_top"] if top == 2 else None, ref["hn"], ref["grads"], ref["d_xc"], L)
    have = named_tensors(hs_top.detach().cpu() if top == 2 else None, hn.detach().cpu(), [p.grad.cpu() for p in ps],
                         xcd.grad.cpu() if xcd is not None else None, L)
    bad = compare(have, want, BF16, label)
    assert not bad, bad


@pytest.mark.parametrize("shape", [(1024, 2, 80, 0, 256, 2), (1024, 3, 80, 32, 256, 2), (1030, 2, 0, 64, 256, 2)])
def test_partial_dh_backward_vs_oracle(hb, shape):
    _check(hb, "rs B%d T%d I%d Ic%d H%d L%d" % shape, shape, RS)


def test_final_state_gradient_only(hb):
    """top = 0: d_hn without d_hs_top."""
    _check(hb, "rs top0 B1024 T2", (1024, 2, 80, 0, 256, 2), RS, top=0)


def test_output_gradient_only(hb):
    """Only g_out: d_hs_top without a gradient of the final states (d_hn is all zeros)."""
    _check(hb, "rs g_out only B1024 T2", (1024, 2, 80, 0, 256, 2), RS, use_hn=False)


@pytest.mark.parametrize("shape", [(16, 2, 80, 0, 256, 2), (300, 2, 40, 0, 128, 2)])
def test_join_of_the_contraction_split_kernels(hb, shape):
    _check(hb, "ks B%d T%d I%d Ic%d H%d L%d" % shape, shape, KS)


def test_repeated_backward_on_one_armed_block(hb):
    """Launch numbers beyond the first on one armed sync block: the same graph's backward three times (retain_graph), each against
    the oracle (not bitwise: the weight gradients use f32 atomics).  Then the ticket words: one forward launch and 3 x 2 backward
    launches took 32 tickets each of every XCD's counter, each counter on a 128-byte line of its own; the old ticket words
    (16..23) stay 0."""
    shape = (1024, 2, 80, 0, 256, 2)
    B, T, I, Ic, H, L = shape
    x, xc, params, g_out, g_hn, ref = _case(shape, True)
    ps, xcd, hs_top, hn, got_form = _forward(hb, x, xc, T, params, 2)
    assert got_form == RS, got_form
    lp = hb.LSTM_WORKSPACES[-1]
    loss = (hn * g_hn.cuda()).sum() + (hs_top * g_out.cuda()).sum()
    want = named_tensors(None, None, ref["grads"], None, L)
    for rep in range(3):
        for p in ps:
            p.grad = None
        loss.backward(retain_graph=True)
        hb.flush_param_grads()
        torch.cuda.synchronize()
        assert hb.lstm_sync_status() == 0, "a persistent recurrence launch gave up (repetition %d)" % rep
        bad = compare(named_tensors(None, None, [p.grad.cpu() for p in ps], None, L), want, BF16, "rs repeat %d" % rep)
        assert not bad, bad
    words = lp[:3072 * 4].view(torch.int32).cpu()
    tickets = [int(words[TICKETS + TICKET_STRIDE * xcd_]) for xcd_ in range(8)]
    print("ticket words:", tickets)
    assert tickets == [32 * (1 + 3 * 2)] * 8, tickets
    assert not words[OLD_TICKETS:OLD_TICKETS + 8].any(), words[OLD_TICKETS:OLD_TICKETS + 8]
