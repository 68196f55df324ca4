"""Float64 K5 (the discriminative log-sum-exp cross-entropy over the mu2 table, simple_fhvae.py:119-122) with the arithmetic of each
HIP form, forward and backward written out (no autograd: the bf16 backward rounds at points the forward's graph does not have).

    logit[b,s] = -c |q_b - t_s|^2,   CE = mean_b (lse_b - logit[b, y_b]),   lse_b = log sum_s exp(logit[b,s])
    w[b,s] = g (p[b,s] - onehot(y_b)),  p = exp(logit - rmax) / rsum,  dq_b = -2c sum_s w (q_b - t_s),  dt_s = 2c sum_b w (q_b - t_s)
with g = gscale * gmul (an f32 product, csrc/loss.hip:572 and disc_mfma.hip:69), (rmax, rsum) the forward's per-query statistics.

Modes (each names the kernel lines it models):
  direct    the VALU kernels, loss.hip:345-374 (forward), 558-603 (dq), 608-648 (dtable): the own row is one of the logits.  Also the
            own-row terms of every form: loss.hip:401-419 (the direct target logit merged into the row sum) and 430-453
            (disc_own_bwd_kernel, w_own = g (exp(t - rmax) / rsum - 1)).
  expanded  disc_mfma.hip (exact-f32 MFMA, 2c q.t - c|q|^2 - c|t|^2): no rounding points, so in float64 it is the direct form.
            The own row is masked out of the MFMA partials (disc_mfma.hip:226-237) and taken in the direct form.
  split     disc_lp.hip, the bf16 compute mode:
              hi = rb(v), lo = rb(v - hi), round to nearest even as f2bf (disc_lp.hip:30-33, common.h:34);
              cross term q_hi.t_hi + q_hi.t_lo + q_lo.t_hi (disc_lp.hip:284-286), norms exact (:119, :198);
              logit 2c cross - c (|q|^2 + |t|^2) (:290); own row masked (:295-296) and taken in the direct form;
              backward weights w = rb(exp(lg - rmax) (gscale / rsum)) (:133, :314, :330);
              G = sum w (y_hi + y_lo) and W = sum w from the same rounded w (:331-337; MODE 2's streamed side :369-375 with a
              bf16 ones operand), gradient 2c (G - x W) with the f32 x (:436; disc_mfma.hip:529);
              own row: the direct logit and its gradient (disc_own_bwd_kernel), as in the other forms.
rb(v) = v.float().bfloat16().double().

Row shards (row0): the table is rows [row0, row0 + S) of the whole; a query whose target lies outside has tgt = 0 and no own term
(loss.hip:403-406, disc_mfma.hip:81, disc_lp.hip:130), and its backward takes the (rmax, rsum) given, i.e. the merged global ones.

The work goes in chunks of table rows, at most `max_elems` (query, row) pairs at a time (B = 16384 x S = 12500: a few GB).  The
tensors stay on their device: a GPU's float64 (d)gemm is as exact as the CPU's, and much faster at the test sizes.

`_fault` is for the comparator's own tests only (tests/test_disc_oracle_cpu.py): a deliberately wrong variant
  {"no_qlo_thi": True}      split cross term without q_lo.t_hi
  {"W_unrounded": True}     split: W summed from the unrounded weights (G from the rounded ones)
  {"G_no_ylo": True}        split: G = sum w y_hi
  {"own_twice": True}       the own row also in the matrix-core partials (forward sum and backward weights)
  {"own_grad_dropped": True}  no own-row gradient
  {"drop_tail_tile": True}  the last partial 64-row table tile left out (its non-own pairs, forward and backward)
  {"drop_queries": n}       the last n queries produce nothing (lse = tgt = 0, no gradient)
  {"split_from": (q, table)}  split: the bf16 operands of these inputs (the floor measurement moves q and the table by one f32
                            ulp; that would move a lo operand by one bf16 ulp now and then, a 2^-16 step of the split form's own
                            resolution rather than f32 noise)
"""
from typing import Optional

import torch

MODES = ("direct", "expanded", "split")


def rb(v: torch.Tensor) -> torch.Tensor:
    return v.float().bfloat16().double()


def split(v: torch.Tensor):
    hi = rb(v)
    return hi, rb(v - hi)


class _Prep:
    """The float64 operands of one problem in the form `mode` uses."""

    def __init__(self, q, table, idx, c, mode, row0, fault, max_elems):
        assert mode in MODES, mode
        self.q, self.t = q.detach().double(), table.detach().double()
        self.B, self.D = self.q.shape
        self.S = self.t.shape[0]
        self.c, self.mode, self.fault = float(c), mode, fault
        self.loc = idx.detach().to(self.q.device).long() - int(row0)
        self.inside = (self.loc >= 0) & (self.loc < self.S)
        self.qn, self.tn = (self.q * self.q).sum(1), (self.t * self.t).sum(1)
        if mode == "split":
            qs, ts = fault.get("split_from", (self.q, self.t))
            self.qh, self.ql = split(qs.detach().to(self.q.device).double())
            self.th, self.tl = split(ts.detach().to(self.q.device).double())
        # the own (direct-form) logit of every query whose target is in this table
        y = self.loc.clamp(0, self.S - 1)
        self.own = torch.where(self.inside, -self.c * ((self.q - self.t[y]) ** 2).sum(1), torch.zeros_like(self.qn))
        self.step = max(1, int(max_elems) // max(self.B, 1))
        self.alive = torch.ones(self.B, dtype=torch.bool, device=self.q.device)
        if fault.get("drop_queries"):
            self.alive[self.B - int(fault["drop_queries"]):] = False
        self.tail0 = (self.S // 64) * 64 if fault.get("drop_tail_tile") else self.S

    def logits(self, s0, s1):
        """The non-own logits of rows [s0, s1): the form's arithmetic, own pairs (and faulted-out pairs) at -inf."""
        c = self.c
        if self.mode == "split":
            th, tl = self.th[s0:s1], self.tl[s0:s1]
            cross = self.qh @ th.T + self.qh @ tl.T
            if not self.fault.get("no_qlo_thi"):
                cross = cross + self.ql @ th.T
        else:
            cross = self.q @ self.t[s0:s1].T
        lg = 2 * c * cross - c * (self.qn[:, None] + self.tn[None, s0:s1])
        if not self.fault.get("own_twice"):
            hit = self.inside & (self.loc >= s0) & (self.loc < s1)
            b = hit.nonzero().squeeze(1)
            lg[b, self.loc[b] - s0] = -float("inf")
        if self.tail0 < s1:
            lg[:, max(self.tail0, s0) - s0:] = -float("inf")
        lg[~self.alive] = -float("inf")
        return lg

    def chunks(self):
        for s0 in range(0, self.S, self.step):
            yield s0, min(self.S, s0 + self.step)


def disc_ref_fwd(q, table, idx, c, mode="direct", row0=0, max_elems=1 << 25, _fault: Optional[dict] = None) -> dict:
    """q (B,D), table (S,D) f32; idx (B,) global target rows.  Returns float64 tensors on q's device: rmax, rsum (the statistics
    the backward takes; rmax = the largest logit), lse = rmax + log rsum, tgt (0 off the shard), ce = mean(lse - tgt)."""
    P = _Prep(q, table, idx, c, mode, row0, _fault or {}, max_elems)
    inf = float("inf")
    m = torch.where(P.inside, P.own, torch.full_like(P.own, -inf))
    s = P.inside.double()
    for s0, s1 in P.chunks():
        lg = P.logits(s0, s1)
        mn = torch.maximum(m, lg.max(1).values)
        ref = torch.where(torch.isfinite(mn), mn, torch.zeros_like(mn))
        s = s * torch.exp(m - ref) + torch.exp(lg - ref[:, None]).sum(1)
        m = mn
    lse = m + torch.log(s)
    tgt = P.own.clone()
    lse[~P.alive], tgt[~P.alive] = 0.0, 0.0
    return {"rmax": m, "rsum": s, "lse": lse, "tgt": tgt, "ce": (lse - tgt).mean()}


def disc_ref_bwd(q, table, idx, c, rmax, rsum, gscale, gmul, mode="direct", row0=0, tgt=None, max_elems=1 << 25,
                 _fault: Optional[dict] = None) -> dict:
    """The backward of the kernels given the forward's statistics (rmax, rsum: the kernel's own, f32) and the upstream gradient
    gscale (the device scalar) * gmul.  tgt: the kernel's f32 target logit.  With it, the own-row weight is taken in f32 as every
    form's kernel takes it (loss.hip:444-445, 590, 636): g (exp(tgt - rmax) / rsum - 1), with the bit-identical logit the forward
    produced (loss.hip:401-402), so that p_own is exactly 1 / rsum where the own row is the maximum; in float64 the cancellation
    p_own - 1 would carry the f32 resolution of rmax (2^-24 |rmax|) into rows whose other weights have underflowed.  Without it
    (the float64 statistics of disc_ref_fwd) the weight is float64.  Returns float64 dq (B,D) and dt (S,D): this table's
    contributions only (a shard's)."""
    fault = _fault or {}
    P = _Prep(q, table, idx, c, mode, row0, fault, max_elems)
    dev = P.q.device
    g32 = torch.tensor(float(gscale), dtype=torch.float32) * torch.tensor(float(gmul), dtype=torch.float32)
    g = g32.item()
    rmax64, rsum64 = rmax.detach().to(dev).double(), rsum.detach().to(dev).double()  # (the kernel's f32 values are exact here)
    rmax32, rsum32 = rmax64.float(), rsum64.float()
    lp = mode == "split"
    # the weight's factor after the exp: g / rsum (the f32 quotient of the kernels in the split form)
    f = (g32.to(dev) / rsum32).double() if lp else g / rsum64
    if lp:
        qy = P.qh if fault.get("G_no_ylo") else P.qh + P.ql
        ty = P.th if fault.get("G_no_ylo") else P.th + P.tl
    else:
        qy, ty = P.q, P.t
    G = torch.zeros_like(P.q)
    W = torch.zeros_like(P.qn)
    dt = torch.zeros_like(P.t)
    # the kernels' rmax is one of their own f32 logits bit for bit (loss.hip:366-368, disc_mfma.hip:244-247, disc_lp.hip:300-303), so
    # the weight of the row that set it is exactly g / rsum there; the oracle's float64 logit of that row differs from rmax by the
    # kernel's f32 error (2^-24 of the row scale, a few times over), and would flip the rounding of that dominant weight now and then
    snap = 2.0 ** -18 * P.c * (P.qn + P.tn.max())
    for s0, s1 in P.chunks():
        lg = P.logits(s0, s1)
        arg = lg - rmax64[:, None]
        arg = torch.where(arg.abs() <= snap[:, None], torch.zeros_like(arg), arg)
        w = torch.exp(arg) * f[:, None]
        wr = rb(w) if lp else w
        G += wr @ ty[s0:s1]
        W += (w if fault.get("W_unrounded") else wr).sum(1)
        Wt = (w if fault.get("W_unrounded") else wr).sum(0)
        dt[s0:s1] = 2 * P.c * (wr.T @ qy - P.t[s0:s1] * Wt[:, None])
    dq = 2 * P.c * (G - P.q * W[:, None])
    if not fault.get("own_grad_dropped"):
        b = (P.inside & P.alive).nonzero().squeeze(1)
        y = P.loc[b]
        if tgt is not None:  # f32, from the kernel's own target logit
            p = torch.exp(tgt.detach().to(dev).float()[b] - rmax32[b]) / rsum32[b]
            wo = (g32.to(dev) * (p - 1.0)).double()
        else:
            wo = g * (torch.exp(P.own[b] - rmax64[b]) / rsum64[b] - 1.0)
        diff = P.q[b] - P.t[y]
        dq.index_add_(0, b, -2 * P.c * wo[:, None] * diff)
        dt.index_add_(0, y, 2 * P.c * wo[:, None] * diff)
    return {"dq": dq, "dt": dt}
