"""float64 oracle of the three matrix-product kernels (csrc/proj.hip, csrc/wgrad.hip, the generic engine of csrc/gemm.hip /
csrc/gemm_core.h behind hip_binding.linear).  Device-agnostic: the results live where the operands live.

Operands are taken AS GIVEN (already bf16-rounded where the kernel takes bf16) and in the layout the kernel reads them:
  KC ("contraction contiguous"):  A is [M, K], B is [N, K]   (activations, nn.Linear weights)
  KM ("contraction is the row"):  A is [K, M], B is [K, N]   (dgates / saved states of a weight gradient)
Every product comes with the sum of the absolute values of its terms (absprod = |A| . |B| + |c0| + |bias|): the comparator
(tests/head_elbo_compare.py check_contraction) scales its per-element bound by it."""
import torch


def _mk(t: torch.Tensor, kc: bool) -> torch.Tensor:
    """The operand as [rows, K] in float64."""
    t = t.detach().double()
    return t if kc else t.t()


def contraction(a, b, a_kc=True, b_kc=True, c0=None, bias=None):
    """(C, absprod) with C[m, n] = sum_k A(m, k) B(n, k) (+ c0[m, n]) (+ bias[n]) in float64."""
    A, B = _mk(a, a_kc), _mk(b, b_kc)
    assert A.shape[1] == B.shape[1], (A.shape, B.shape)
    c = A @ B.t()
    ab = A.abs() @ B.abs().t()
    if c0 is not None:
        c = c + c0.detach().double()
        ab = ab + c0.detach().double().abs()
    if bias is not None:
        c = c + bias.detach().double()[None, :]
        ab = ab + bias.detach().double().abs()[None, :]
    return c, ab


def linear_fwd(x, w, b=None, relu=False):
    """y = act(x W^T + b) (simple_fhvae.py:127-134) and the absprod of the pre-activation (a clipped output errs by no more)."""
    y, ab = contraction(x, w, True, True, bias=b)
    return (y.clamp_min(0.0) if relu else y), ab


def linear_bwd(x, w, y, dy, relu=False, dw0=None, db0=None, dx0=None):
    """The backward of linear_fwd from the upstream gradient dy.  The ReLU mask is taken from the y PASSED IN (a GPU test passes
    the kernel's own y: an output within an ulp of 0 must not force loose bounds on everything downstream).  dw0 / db0 / dx0:
    what the sinks held before (the kernels accumulate).  Returns dx, dw, db with a_dx, a_dw (absprod) and a_db (sum_m |g|)."""
    g = dy.detach().double()
    if relu:
        g = torch.where(y.detach() > 0, g, torch.zeros_like(g))
    dx, a_dx = contraction(g, w, True, False, c0=dx0)       # dx[m, k] = sum_n g[m, n] w[n, k]: w is the KM operand
    dw, a_dw = contraction(g, x, False, False, c0=dw0)      # dw[n, k] = sum_m g[m, n] x[m, k]: both KM
    db, a_db = g.sum(0), g.abs().sum(0)
    if db0 is not None:
        db, a_db = db + db0.detach().double(), a_db + db0.detach().double().abs()
    return {"g": g, "dx": dx, "a_dx": a_dx, "dw": dw, "a_dw": a_dw, "db": db, "a_db": a_db}
