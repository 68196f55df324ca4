"""Float64 LSTM forward + BPTT with the bf16 rounding points of the HIP recurrences (hip_binding.lstm_seq, bf16 mode).

Explicit forward and backward (no autograd: the backward rounds at points the forward's graph does not have).  PyTorch's
documented LSTM equations, gate order (i, f, g, o):
    pre_t = [x_t | xc] W_ih^T + h_{t-1} W_hh^T + b_ih + b_hh,  c_t = f c_{t-1} + i g,  h_t = o tanh(c_t).

rb(v) = v.float().bfloat16().double(): f32 first, then round to nearest even (f2bf, csrc/common.h).  The element-wise step
between the contractions is the one definition every schedule calls, lstm_point_fwd / lstm_point_bwd (csrc/lstm_point.h), here
in float64 (its f32 roundings are below what this oracle resolves).  With rounding=True the model is the one every bf16
schedule shares:
  forward   the MFMA operands rb([x_t | xc]), rb(W_ih), rb(h_{t-1}), rb(W_hh) (csrc/lstm.hip cast_operands; the step cells and the
            persistent kernels store rb(h) as the next step's / layer's operand: lstm_cluster.hip pack4(h), lstm_fwd_wr.hip f2bf(h)),
            exact products, unrounded sums and biases; gates, c and h unrounded (hs_top / hn are the f32 h); the gates saved for
            the backward are rb(gates) (pack4 / store_h), c is saved in f32.
  backward  reads rb(saved gates) and the unrounded c;
            dh = external + rb(dg^{l+1}) rb(W_ih^{l+1}) + rb(dg_{t+1}) rb(W_hh)  (from-above term: proj.hip / the generic engine);
            dW = rb(dg)^T rb(operand) (wgrad.hip over the bf16 dgates and saved bf16 states);
            time-constant input: dgsum = sum_t dg (f32, layer 0), dW_xc = dgsum^T xc and d_xc = dgsum W_xc with the f32 xc and
            the f32 master weight (lstm.hip lstm_param_grads, lstm_dxc: launch_gemm(..., FHVAE_F32));
            bias gradients: sums of the unrounded dg (lstm_bwd_layer_rs_kernel, lstm_bwd_layer_kernel and lstm_bwd_ksplit_kernel
            add lstm_point_bwd's dp to dgs before pack4);
            layer 0 with a time-constant input: the column sums of dgsum (lstm.hip lstm_param_grads).
Schedule options (each cites the code that makes it):
  partial_dh_bf16        lstm_bwd_rs.hip (header comment; lstm_bwd_layer_rs_kernel): member m (units [64m, 64m+64)) multiplies its own 256 gate
                         columns of rb(dg_t) by rb(W_hh) for ALL units; the partials for the other members travel as bf16
                         (pack4(acc[rt][j]), j = 1..3), its own stays f32.
  bias_from_rounded_dg   lstm.hip lstm_param_grads: the per-step and large-tile cells leave the bias gradients to launch_colsum over the
                         saved bf16 dgates: sums of rb(dg) (except layer 0 with a time-constant input, which sums dgsum).
  dgsum_from_rounded_dg  lstm.hip lstm_bwd_impl / lstm_cell.hip cell_dgsum_kernel: the large-tile cells build dgsum from the saved bf16 dgates.
rounding=False is a plain float64 LSTM (the oracle of the f32 mode).

`_fault` is for the comparator's own tests only (tests/test_lstm_lp_oracle_cpu.py): a deliberately wrong variant
  {"drop_dc": (t, block)}   the dc carry of 64-unit block `block` dropped at step t (every layer)
  {"bias_rows": n}          only the first n batch rows enter the bias sums
  {"bwd_unrounded_gates": True}  the backward reads the unrounded gates
"""
from typing import Optional, Sequence

import torch


def rb(v: torch.Tensor) -> torch.Tensor:
    return v.float().bfloat16().double()


def lstm_lp_ref(x: Optional[torch.Tensor], xc: Optional[torch.Tensor], params: Sequence[torch.Tensor],
                g_out: Optional[torch.Tensor], g_hn: Optional[torch.Tensor], T: Optional[int] = None, rounding: bool = True,
                partial_dh_bf16: bool = False, bias_from_rounded_dg: bool = False, dgsum_from_rounded_dg: bool = False,
                _fault: Optional[dict] = None) -> dict:
    """x (T,B,I) time-major or None; xc (B,Ic) or None; params flat per layer (w_ih, w_hh, b_ih, b_hh); g_out (T,B,H) or None;
    g_hn (B, L*H) or None.  Returns float64 tensors: hs_top (T,B,H), hn (B,L*H), grads (list like params), d_xc (B,Ic) or None,
    hs_lp (T,B,H): the top layer's bf16 states rb(h) (rounding only)."""
    fault = _fault or {}
    dd = lambda t: None if t is None else t.detach().cpu().double()
    r = rb if rounding else (lambda v: v)
    x, xc, g_out, g_hn = dd(x), dd(xc), dd(g_out), dd(g_hn)
    P = [dd(p) for p in params]
    L = len(P) // 4
    assert len(P) == 4 * L and L >= 1
    H = P[1].shape[1]
    I = x.shape[2] if x is not None else 0
    Ic = xc.shape[1] if xc is not None else 0
    B = x.shape[1] if x is not None else xc.shape[0]
    T = x.shape[0] if x is not None else int(T)
    assert P[0].shape == (4 * H, I + Ic)
    Wi = [r(P[4 * l]) for l in range(L)]
    Wh = [r(P[4 * l + 1]) for l in range(L)]
    bias = [P[4 * l + 2] + P[4 * l + 3] for l in range(L)]
    xcr = r(xc) if Ic else None

    # ---- forward
    inp = []   # per layer: (T,B,K) MFMA operand of W_ih
    gates_s, cs, hs, hs_r = [], [], [], []
    below = None
    for l in range(L):
        if l == 0:
            parts = ([r(x)] if I else []) + ([xcr[None].expand(T, B, Ic)] if Ic else [])
            a = torch.cat(parts, -1)
        else:
            a = below
        inp.append(a)
        proj = (a.reshape(T * B, -1) @ Wi[l].t()).reshape(T, B, 4 * H) + bias[l]
        h = torch.zeros(B, H, dtype=torch.float64)
        c = torch.zeros(B, H, dtype=torch.float64)
        G = torch.empty(T, B, 4 * H, dtype=torch.float64)
        Cs = torch.empty(T, B, H, dtype=torch.float64)
        Hs = torch.empty(T, B, H, dtype=torch.float64)
        for t in range(T):
            pre = proj[t] + r(h) @ Wh[l].t() if t > 0 else proj[t]
            i, f, g, o = (pre[:, k * H:(k + 1) * H] for k in range(4))
            i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
            c = f * c + i * g
            h = o * torch.tanh(c)
            G[t] = torch.cat([i, f, g, o], -1)
            Cs[t], Hs[t] = c, h
        gates_s.append(G if fault.get("bwd_unrounded_gates") else r(G))
        cs.append(Cs)
        hs.append(Hs)
        hs_r.append(r(Hs))
        below = hs_r[l]
    hn = torch.cat([hs[l][T - 1] for l in range(L)], -1)

    # ---- backward, layer by layer from the top (the from-above term of layer l needs all of layer l+1's dg)
    grads = [None] * (4 * L)
    d_xc = None
    dg_above = None
    drop = fault.get("drop_dc")
    for l in reversed(range(L)):
        ext = torch.zeros(T, B, H, dtype=torch.float64)
        if l == L - 1 and g_out is not None:
            ext = ext + g_out
        if dg_above is not None:
            ext = ext + (r(dg_above).reshape(T * B, 4 * H) @ Wi[l + 1]).reshape(T, B, H)
        if g_hn is not None:
            ext[T - 1] = ext[T - 1] + g_hn[:, l * H:(l + 1) * H]
        G, Cs = gates_s[l], cs[l]
        dg = torch.empty(T, B, 4 * H, dtype=torch.float64)
        dc_carry = torch.zeros(B, H, dtype=torch.float64)
        dg_next = None
        for t in reversed(range(T)):
            dh = ext[t].clone()
            if dg_next is not None:
                dh = dh + _recurrent(r(dg_next), Wh[l], H, partial_dh_bf16 and rounding)
            i, f, g, o = (G[t][:, k * H:(k + 1) * H] for k in range(4))
            tc = torch.tanh(Cs[t])
            dc = dh * o * (1 - tc * tc) + dc_carry
            cp = Cs[t - 1] if t > 0 else torch.zeros_like(tc)
            d_o = dh * tc
            dc_carry = dc * f
            if drop is not None and drop[0] == t:
                dc_carry[:, 64 * drop[1]:64 * drop[1] + 64] = 0
            dg[t] = torch.cat([dc * g * i * (1 - i), dc * cp * f * (1 - f), dc * i * (1 - g * g), d_o * o * (1 - o)], -1)
            dg_next = dg[t]
        dgr = r(dg).reshape(T * B, 4 * H)
        a = inp[l].reshape(T * B, -1)
        dw_ih = torch.zeros(4 * H, inp[l].shape[2], dtype=torch.float64)
        dgsum = None
        if l == 0 and Ic:
            dgsum = (r(dg) if dgsum_from_rounded_dg else dg).sum(0)
            dw_ih[:, I:] = dgsum.t() @ xc
            d_xc = dgsum @ P[0][:, I:]
            if I:
                dw_ih[:, :I] = dgr.t() @ a[:, :I]
        else:
            dw_ih = dgr.t() @ a
        dw_hh = dgr.reshape(T, B, 4 * H)[1:].reshape(-1, 4 * H).t() @ hs_r[l][:-1].reshape(-1, H) if T > 1 else \
            torch.zeros(4 * H, H, dtype=torch.float64)
        if dgsum is not None:
            db = dgsum[:fault.get("bias_rows", B)].sum(0)
        else:
            db = (r(dg) if bias_from_rounded_dg else dg)[:, :fault.get("bias_rows", B)].sum((0, 1))
        grads[4 * l:4 * l + 4] = [dw_ih, dw_hh, db, db.clone()]
        dg_above = dg
    return {"hs_top": hs[L - 1], "hn": hn, "grads": grads, "d_xc": d_xc, "hs_lp": hs_r[L - 1] if rounding else None}


def _recurrent(dgr: torch.Tensor, whr: torch.Tensor, H: int, partial: bool) -> torch.Tensor:
    """rb(dg_{t+1}) . rb(W_hh); partial: split by source member, the partials for other members rounded to bf16."""
    if not partial:
        return dgr @ whr
    assert H % 64 == 0
    out = torch.zeros(dgr.shape[0], H, dtype=torch.float64)
    for m in range(H // 64):
        cols = torch.cat([torch.arange(g * H + 64 * m, g * H + 64 * m + 64) for g in range(4)])
        p = dgr[:, cols] @ whr[cols]
        pr = rb(p)
        pr[:, 64 * m:64 * m + 64] = p[:, 64 * m:64 * m + 64]
        out = out + pr
    return out
