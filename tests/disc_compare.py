"""One comparator for the K5 kernels (hip_binding.raw_disc_fwd / raw_disc_bwd) against the float64 oracle of their own arithmetic
(oracle/disc_ref.py), with one set of constants per form shared by every case: tests/test_disc_oracle_gpu.py checks the kernels
with it, tests/test_disc_oracle_cpu.py checks that it rejects the errors a kernel could hide.

Forward, per query b, against the row scale sc_b = c (|q_b|^2 + max_s |t_s|^2) (a logit's f32 resolution is ~2^-24 of it):
  lse      max_b |lse_b - lse*_b| / sc_b   (lse = rmax + log rsum: the split between the two is the kernel's choice)
  tgt      max_b |tgt_b - tgt*_b| / sc_b
  ce       |CE - CE*| / mean_b sc_b
  mean     mean_b of (lse + tgt error) / sc_b
Gradients, per row r, against the unit-weight scale G0 = 2c |g| (max |q_b| + max |t_s|) (the size of the gradient one pair of
weight g leaves; it stays put where the softmax underflows and the gradients vanish):
  max / mean   over rows of |row - row*| / (|row*| + floor G0): the error relative to the row's own norm, so a small row that
               misses its far-row contributions, or gets its own row twice, counts as much as a large one.
Bins: forward, (256-query tile x 1024-row table chunk of the target); dq, 256-query tiles; dtable, 64-row table tiles.  The worst
bin's mean may not exceed LOCAL_RATIO x the median bin's mean + a floor (mean / gbin): an error confined to a ragged query tile, a partial table
tile or one chunk stands out there long before it moves the tensor-wide numbers.

The floor of the comparison is the oracle against itself with q and the table moved by one f32 ulp in a random half of their
entries (test_disc_oracle_cpu.py::test_floor_is_below_the_constants measures it; numbers below).  What remains between a kernel
and its oracle is f32 arithmetic: the accumulation order of the cross term and of the row sums, __expf, and, in the split form,
the bf16 rounding of a weight that such a difference flips now and then (one weight moved by 2^-8: a dq / dtable row dominated
by that weight moves by ~4e-3 of its norm).
"""
import torch

LOCAL_RATIO = 8.0
TCHUNK = 1024

# The measured floor (test_disc_oracle_cpu.py::test_floor_is_below_the_constants: B = 300 and 1000, S = 4633 and 9000, D = 32,
# the four regimes, random and edge targets):
#   forward, every form  lse 1.2e-7, tgt 1.2e-7, ce 1.8e-8, mean 3e-8
#   direct / expanded    gradient rows max 9.6e-6 (unrelated), 7.1e-5 (separated), mean 1e-6 / 5e-6
#   split                gradient rows max 7.6e-3 (a dtable row whose largest weight's bf16 rounding flipped), mean 1e-6; one
#                        such row in a 64-row bin: a bin mean of 1.2e-4 (the bin floor gbin)
#   converged and exact: zero gradients (every far weight underflows, p_own = 1 exactly) and forward errors of 1e-11.
# The kernels on an MI355X (tests/test_disc_oracle_gpu.py, every case): forward lse 2.1e-7, tgt 2.1e-7, ce 3.6e-8, mean 5.3e-8 in
# every form; gradient rows max / mean direct 5.5e-4 / 8.4e-6, expanded 2.4e-3 / 1.2e-5 (f32 cancellation in 2c (G - t W) of a
# dtable row with a small net gradient), split 7.1e-3 / 1.5e-5 (worst 64-row bin 1.8e-4); the constants sit above both.
DIRECT = {"lse": 6e-7, "tgt": 6e-7, "ce": 2e-7, "mean": 1.5e-7, "gmax": 2e-3, "gmean": 5e-5, "gbin": 1e-4, "floor": 1e-6}
EXPANDED = dict(DIRECT, gmax=1e-2, gbin=2e-4)
SPLIT = {"lse": 6e-7, "tgt": 6e-7, "ce": 2e-7, "mean": 1.5e-7, "gmax": 2e-2, "gmean": 5e-5, "gbin": 5e-4, "floor": 1e-6}
CONSTS = {"direct": DIRECT, "expanded": EXPANDED, "split": SPLIT}


def _bin_stats(err: torch.Tensor, ids: torch.Tensor) -> tuple:
    """(worst bin mean, median bin mean) of err over the bins ids (non-empty bins only)."""
    ids = ids.reshape(-1).long()
    n = int(ids.max().item()) + 1
    s = torch.bincount(ids, weights=err.reshape(-1), minlength=n)
    k = torch.bincount(ids, minlength=n).double()
    bm = (s / k.clamp_min(1))[k > 0]
    return bm.max().item(), bm.median().item()


def row_scale(q, table, c) -> torch.Tensor:
    q, table = q.detach().double(), table.detach().double()
    return c * ((q * q).sum(1) + (table * table).sum(1).max())


def grad_scale(q, table, c, g) -> float:
    q, table = q.detach().double(), table.detach().double()
    return 2 * c * abs(float(g)) * (q.norm(dim=1).max().item() + table.norm(dim=1).max().item())


def measure_fwd(got: dict, want: dict, sc: torch.Tensor, idx: torch.Tensor) -> dict:
    """got: the kernel's rmax, rsum, tgt (f32) and ce (optional); want: disc_ref_fwd's dict; sc: row_scale."""
    dev = sc.device
    lse = got["rmax"].detach().to(dev).double() + torch.log(got["rsum"].detach().to(dev).double())
    el = (lse - want["lse"].to(dev)).abs() / sc
    et = (got["tgt"].detach().to(dev).double() - want["tgt"].to(dev)).abs() / sc
    B = sc.shape[0]
    tile = torch.arange(B, device=dev) // 256
    chunk = idx.to(dev).long().clamp_min(0) // TCHUNK
    ids = tile * (int(chunk.max().item()) + 1) + chunk
    e = el + et
    bmax, bmed = _bin_stats(torch.nan_to_num(e, nan=1e30, posinf=1e30), ids)
    st = {"finite": bool(torch.isfinite(lse).all() and torch.isfinite(got["tgt"]).all()), "lse": el.max().item(),
          "tgt": et.max().item(), "mean": e.mean().item(), "bin_max": bmax, "bin_med": bmed}
    if got.get("ce") is not None:
        st["ce"] = abs(float(got["ce"]) - want["ce"].item()) / sc.mean().item()
    return st


def measure_grad(got: torch.Tensor, want: torch.Tensor, G0: float, floor: float, rows_per_bin: int) -> dict:
    want = want.double()
    got = got.detach().to(want.device).double()
    assert got.shape == want.shape, (got.shape, want.shape)
    r = (got - want).norm(dim=1) / (want.norm(dim=1) + floor * G0)
    ids = torch.arange(r.shape[0], device=r.device) // rows_per_bin
    bmax, bmed = _bin_stats(torch.nan_to_num(r, nan=1e30, posinf=1e30), ids)
    return {"finite": bool(torch.isfinite(got).all()), "max": r.max().item(), "mean": r.mean().item(), "bin_max": bmax,
            "bin_med": bmed}


def fwd_failures(st: dict, k: dict) -> list:
    bad = [] if st["finite"] else ["not finite"]
    for n in ("lse", "tgt", "ce", "mean"):
        if n in st and not st[n] <= k[n]:
            bad.append("%s %.3g > %.3g" % (n, st[n], k[n]))
    lim = LOCAL_RATIO * st["bin_med"] + k["mean"]
    if not st["bin_max"] <= lim:
        bad.append("local: worst bin %.3g > %.3g (median bin %.3g)" % (st["bin_max"], lim, st["bin_med"]))
    return bad


def grad_failures(st: dict, k: dict) -> list:
    bad = [] if st["finite"] else ["not finite"]
    if not st["max"] <= k["gmax"]:
        bad.append("max %.3g > %.3g" % (st["max"], k["gmax"]))
    if not st["mean"] <= k["gmean"]:
        bad.append("mean %.3g > %.3g" % (st["mean"], k["gmean"]))
    lim = LOCAL_RATIO * st["bin_med"] + k["gbin"]
    if not st["bin_max"] <= lim:
        bad.append("local: worst bin %.3g > %.3g (median bin %.3g)" % (st["bin_max"], lim, st["bin_med"]))
    return bad


def fmt_fwd(st: dict) -> str:
    return "lse %.2e tgt %.2e ce %s mean %.2e bin %.2e/med %.2e" % (
        st["lse"], st["tgt"], ("%.2e" % st["ce"]) if "ce" in st else "-", st["mean"], st["bin_max"], st["bin_med"])


def fmt_grad(st: dict) -> str:
    return "max %.2e mean %.2e bin %.2e/med %.2e" % (st["max"], st["mean"], st["bin_max"], st["bin_med"])


def compare_fwd(got: dict, want: dict, q, table, idx, c, consts: dict, label: str = "", quiet: bool = False) -> list:
    st = measure_fwd(got, want, row_scale(q, table, c).to(want["lse"].device), idx)
    bad = fwd_failures(st, consts)
    if not quiet:
        print("%s fwd    %s%s" % (label, fmt_fwd(st), ("  FAIL: " + "; ".join(bad)) if bad else ""))
    return ["%s fwd: %s" % (label, b) for b in bad]


def compare_bwd(got: dict, want: dict, q, table, c, g, consts: dict, label: str = "", quiet: bool = False) -> list:
    """got / want: {"dq": (B,D), "dt": (S,D)} (either may be missing from got)."""
    G0 = grad_scale(q, table, c, g)
    bad = []
    for name, rows in (("dq", 256), ("dt", 64)):
        if got.get(name) is None:
            continue
        st = measure_grad(got[name], want[name], G0, consts["floor"], rows)
        f = grad_failures(st, consts)
        if not quiet:
            print("%s %-6s %s%s" % (label, name, fmt_grad(st), ("  FAIL: " + "; ".join(f)) if f else ""))
        bad += ["%s %s: %s" % (label, name, x) for x in f]
    return bad


REGIMES = ("unrelated", "converged", "separated", "exact")
PATTERNS = ("random", "shared", "edges")


def edge_rows(S: int) -> torch.Tensor:
    """Rows 0 and S - 1 and the rows +-1 around every 32-, 64- and 256-row boundary (each boundary row itself included)."""
    rows = {0, S - 1}
    for k in range(32, S, 32):
        rows.update((k - 1, k, k + 1))
    return torch.tensor(sorted(r for r in rows if 0 <= r < S), dtype=torch.int64)


def make_inputs(B: int, S: int, D: int, regime: str, pattern: str, seed: int):
    """Seeded CPU f32 (q, table) and int64 idx of one K5 problem.
    regime  unrelated: q and the table N(0,1), unrelated (the start of training);
            converged: table 10 N(0,1), q = t[idx] + 1e-3 N(0,1) (where training goes, at 10x norms);
            separated: table 3 N(0,1); even queries t[idx] + 0.5 N(0,1), odd ones 3 N(0,1): most exp() underflow;
            exact:     q = t[idx] exactly (own logit 0).
    pattern random: uniform targets with duplicates; shared: the first 256 queries share one target; edges: the targets cycle
            through edge_rows(S) (a random order), the rest uniform."""
    g = torch.Generator().manual_seed(seed)
    scale = {"unrelated": 1.0, "converged": 10.0, "separated": 3.0, "exact": 1.0}[regime]
    table = torch.randn(S, D, generator=g) * scale
    idx = torch.randint(0, S, (B,), generator=g)
    if B > 1:
        idx[1] = idx[0]
    if pattern == "shared":
        idx[: min(B, 256)] = int(torch.randint(0, S, (1,), generator=g))
    elif pattern == "edges":
        e = edge_rows(S)
        e = e[torch.randperm(e.numel(), generator=g)]
        n = min(B, e.numel())
        idx[:n] = e[:n]
        if B > n:
            idx[n:2 * n] = e[: min(n, B - n)]
    if regime == "unrelated":
        q = torch.randn(B, D, generator=g)
    elif regime == "converged":
        q = table[idx] + 1e-3 * torch.randn(B, D, generator=g)
    elif regime == "separated":
        q = table[idx] + 0.5 * torch.randn(B, D, generator=g)
        q[1::2] = 3.0 * torch.randn(B // 2, D, generator=g)
    else:
        q = table[idx].clone()
    return q.contiguous(), table.contiguous(), idx
