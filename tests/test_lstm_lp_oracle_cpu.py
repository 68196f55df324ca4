"""The float64 rounding-model oracle of the LSTM recurrences (oracle/lstm_lp_ref.py) and the comparator of the GPU checks
(tests/lstm_lp_compare.py), on the CPU: the oracle without rounding is torch.nn.LSTM in float64; with rounding it stays within
the bf16 bounds of the f32 torch.nn.LSTM; and the comparator, with the constants the GPU file uses, rejects errors at bf16-noise
level and errors confined to one unit block, one step or one tail of rows."""
import pytest
import torch

from lstm_lp_compare import BF16, compare, make_inputs as _inputs, named_tensors
from oracle.lstm_lp_ref import lstm_lp_ref, rb


def _torch_lstm(x, xc, params, g_out, g_hn, L, H, dtype):
    """torch.nn.LSTM (autograd) on the same inputs, time-major: hs_top, hn, parameter gradients, d_xc."""
    T, B = g_out.shape[:2]
    I = x.shape[2] if x is not None else 0
    Ic = xc.shape[1] if xc is not None else 0
    lstm = torch.nn.LSTM(I + Ic, H, L).to(dtype)
    names = [n + "_l%d" % l for l in range(L) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    with torch.no_grad():
        for n, p in zip(names, params):
            getattr(lstm, n).copy_(p)
    xcl = xc.to(dtype).clone().requires_grad_(True) if Ic else None
    parts = ([x.to(dtype)] if I else []) + ([xcl[None].expand(T, B, Ic)] if Ic else [])
    out, (hn, _) = lstm(torch.cat(parts, -1))
    hn = torch.cat([hn[l] for l in range(L)], -1)
    ((out * g_out.to(dtype)).sum() + (hn * g_hn.to(dtype)).sum()).backward()
    return out.detach(), hn.detach(), [getattr(lstm, n).grad for n in names], (xcl.grad if Ic else None)


@pytest.mark.parametrize("B,T,I,Ic,H,L", [(5, 4, 6, 0, 8, 1), (7, 3, 6, 4, 8, 2), (6, 5, 0, 5, 16, 3), (4, 1, 3, 2, 8, 2),
                                          (9, 6, 10, 0, 64, 2), (3, 2, 0, 3, 12, 1)])
def test_unrounded_oracle_is_torch_lstm_f64(B, T, I, Ic, H, L):
    x, xc, params, g_out, g_hn = _inputs(B, T, I, Ic, H, L, B + 10 * T + L)
    want = _torch_lstm(x, xc, params, g_out, g_hn, L, H, torch.float64)
    got = lstm_lp_ref(x, xc, params, g_out, g_hn, T=T, rounding=False)
    pairs = [(got["hs_top"], want[0]), (got["hn"], want[1])] + list(zip(got["grads"], want[2]))
    if Ic:
        pairs.append((got["d_xc"], want[3]))
    for u, v in pairs:
        assert u.shape == v.shape
        assert (u - v).abs().max().item() <= 1e-10 * max(1.0, v.abs().max().item())


def test_rounded_oracle_within_bf16_of_f32_lstm():
    """The rounding model is not off by more than bf16 allows: today's bounds of the bf16 kernels against the f32 torch.nn.LSTM
    (3e-2 of the tensor's max forward, 6e-2 for gradients, mean 2.5e-3, signed mean 5e-4)."""
    B, T, I, Ic, H, L = 64, 12, 20, 8, 128, 2
    x, xc, params, g_out, g_hn = _inputs(B, T, I, Ic, H, L, 5)
    f32 = _torch_lstm(x, xc, params, g_out, g_hn, L, H, torch.float32)
    o = lstm_lp_ref(x, xc, params, g_out, g_hn, partial_dh_bf16=True)
    pairs = [(o["hs_top"], f32[0], 3e-2), (o["hn"], f32[1], 3e-2), (o["d_xc"], f32[3], 6e-2)]
    pairs += [(u, v, 6e-2) for u, v in zip(o["grads"], f32[2])]
    for u, v, tol in pairs:
        d, s = u - v.double(), v.abs().max().item()
        assert d.abs().max().item() <= tol * s and d.abs().mean().item() <= 2.5e-3 * s and abs(d.mean().item()) <= 5e-4 * s


# the sharpness cases: the schedule of the rows-form partial-dh backward at H = 256 (B = 256: 8 clusters of 32 rows)
_B, _T, _I, _H, _L = 256, 20, 80, 256, 2


@pytest.fixture(scope="module")
def sharp():
    x, xc, params, g_out, g_hn = _inputs(_B, _T, _I, 0, _H, _L, 11)
    ref = lstm_lp_ref(x, None, params, g_out, g_hn, partial_dh_bf16=True)
    return (x, params, g_out, g_hn), named_tensors(ref["hs_top"], ref["hn"], ref["grads"], None, _L)


def _variant(sharp, which):
    x, params, g_out, g_hn = sharp[0]
    if which == "f32_torch_lstm":
        o = _torch_lstm(x, None, params, g_out, g_hn, _L, _H, torch.float32)
        return named_tensors(o[0], o[1], o[2], None, _L)
    kw = {"partial_dh_bf16": True}
    if which == "partial_dh_toggled":
        kw["partial_dh_bf16"] = False
    elif which == "bias_from_rounded_dg":
        kw["bias_from_rounded_dg"] = True
    elif which == "bwd_unrounded_gates":
        kw["_fault"] = {"bwd_unrounded_gates": True}
    elif which == "dc_carry_dropped":
        kw["_fault"] = {"drop_dc": (_T // 2, 2)}
    elif which == "ragged_tail_bias":
        kw["_fault"] = {"bias_rows": _B - 16}
    o = lstm_lp_ref(x, None, params, g_out, g_hn, **kw)
    return named_tensors(o["hs_top"], o["hn"], o["grads"], None, _L)


def test_comparator_accepts_the_oracle_itself(sharp):
    assert compare(sharp[1], sharp[1], BF16, "self") == []


def test_comparator_accepts_f32_level_noise(sharp):
    """The floor the constants are set against: the oracle with its biases and g_out perturbed at f32 level (what a different
    f32 accumulation order does to the kernels' sums) passes against itself.  The one-ulp flips of rb(h) / rb(gate) / rb(dg)
    this causes are the whole of the measured kernel-vs-oracle difference on the GPU."""
    x, params, g_out, g_hn = sharp[0]
    g = torch.Generator().manual_seed(3)
    p2 = [q.double() + (torch.randn(q.shape, generator=g, dtype=torch.float64) * 3e-7 if q.dim() == 1 else 0) for q in params]
    go2 = g_out.double() * (1 + torch.randn(g_out.shape, generator=g, dtype=torch.float64) * 1e-7)
    o = lstm_lp_ref(x, None, p2, go2, g_hn, partial_dh_bf16=True)
    assert compare(named_tensors(o["hs_top"], o["hn"], o["grads"], None, _L), sharp[1], BF16, "f32-noise") == []


# Not in this list: partial_dh_bf16 toggled and the bias gradients summed from rb(dg).  Against the oracle they differ by mean
# 2e-5 .. 8e-5 of scale, the size of the f32-level noise above: a comparison that lets the GPU's flips of rb(.) propagate cannot
# tell them apart from a correct kernel.
@pytest.mark.parametrize("which", ["f32_torch_lstm", "bwd_unrounded_gates", "dc_carry_dropped", "ragged_tail_bias"])
def test_comparator_rejects(sharp, which):
    bad = compare(_variant(sharp, which), sharp[1], BF16, which)
    assert bad, "%s passed the bf16 comparator" % which


def test_rb_is_round_to_nearest_even_through_f32():
    # 1 + 2^-8 is the midpoint between 1 and 1 + 2^-7: ties to the even mantissa (1); a hair above rounds up
    v = torch.tensor([1 + 2 ** -8, 1 + 2 ** -8 + 2 ** -20, 1 + 3 * 2 ** -8], dtype=torch.float64)
    assert rb(v).tolist() == [1.0, 1 + 2 ** -7, 1 + 2 ** -6]
