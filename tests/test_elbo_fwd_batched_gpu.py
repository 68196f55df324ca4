"""elbo_fwd_kernel (csrc/loss.hip) at the shapes at which its pass loop changes shape: all five outputs against the float64 formula
(simple_fhvae.py:105-116), element-wise at the tolerance of tests/test_config_parity_gpu.py (close_elementwise: 1e-4 relative,
1e-5 absolute).  Shapes: the configs' frame (T = 20, F = 80: 400 16-byte pieces, seven passes of a wave), one pass with idle lanes
(T = 1, F = 8), a row length that is no divisor of 64 (F = 84: 21 pieces per row), F = 82 (no multiple of 4: the scalar path) and
600 pieces (ten passes).  Time-major and batch-major strides, per-row and scalar num_segs.  Written for a form of the kernel that
loads its passes in batches (measured, not faster, not in the tree); it holds for the kernel as it is and
for any such form."""
import pytest
import torch

pytestmark = pytest.mark.gpu

NAMES = ["lower_bound", "log_px_z", "neg_kld_z1", "neg_kld_z2", "log_pmu2"]
D1, D2 = 32, 16


@pytest.fixture(scope="module")
def hb():
    import build_ext

    build_ext.build(verbose=False)
    import hip_binding

    hip_binding.load_library()
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return hip_binding


def _ref(x, x_mu, x_lv, z1_mu, z1_lv, z2_mu, z2_lv, mu2, ns):
    """float64, batch-major x (B,T,F)."""
    x, x_mu, x_lv, z1_mu, z1_lv, z2_mu, z2_lv, mu2 = (t.double() for t in (x, x_mu, x_lv, z1_mu, z1_lv, z2_mu, z2_lv, mu2))
    log2pi = 1.8378770664093453
    pz2_lv = float(torch.tensor(0.25, dtype=torch.float32).log())  # float32(log 0.25), as the kernel's constant
    v2 = float(torch.tensor(pz2_lv, dtype=torch.float32).exp())    # expf of it, in f32
    px = (-0.5 * (log2pi + x_lv + (x - x_mu) ** 2 / x_lv.exp())).sum((1, 2))
    k1 = 0.5 * (1 + z1_lv - z1_mu ** 2 - z1_lv.exp()).sum(1)
    k2 = 0.5 * (1 + z2_lv - pz2_lv - ((z2_mu - mu2) ** 2 + z2_lv.exp()) / v2).sum(1)
    pm = (-0.5 * (log2pi + mu2 ** 2)).sum(1)
    return {"lower_bound": px + k1 + k2 + pm / ns, "log_px_z": px, "neg_kld_z1": k1, "neg_kld_z2": k2, "log_pmu2": pm}


_INPUTS = {}


def _inputs(B, T, F):
    if (B, T, F) not in _INPUTS:
        g = torch.Generator().manual_seed(B * 1000 + T * 10 + F)
        x, x_mu = torch.randn(B, T, F, generator=g), torch.randn(B, T, F, generator=g)
        x_lv = torch.randn(B, T, F, generator=g) * 0.5
        z = [torch.randn(B, D1, generator=g), torch.randn(B, D1, generator=g) * 0.5, torch.randn(B, D2, generator=g),
             torch.randn(B, D2, generator=g) * 0.5, torch.randn(B, D2, generator=g)]
        ns = torch.randint(20, 200, (B,), generator=g)
        want = {"row": _ref(x, x_mu, x_lv, *z, ns.double()), "scalar": _ref(x, x_mu, x_lv, *z, 37.0)}
        _INPUTS[(B, T, F)] = (x, x_mu, x_lv, z, ns, want)
    return _INPUTS[(B, T, F)]


@pytest.mark.parametrize("time_major", [True, False])
@pytest.mark.parametrize("B,T,F", [(5, 20, 80), (3, 1, 8), (7, 13, 84), (4, 20, 82), (2, 30, 80)])
def test_elbo_fwd_vs_float64(hb, B, T, F, time_major):
    x, x_mu, x_lv, z, ns, want = _inputs(B, T, F)
    if time_major:
        lay = lambda t: t.transpose(0, 1).contiguous().cuda()
        strides = (F, B * F)
    else:
        lay = lambda t: t.contiguous().cuda()
        strides = (T * F, F)
    xd, md, ld = lay(x), lay(x_mu), lay(x_lv)
    zd = [t.cuda() for t in z]
    bad = []
    for label, nsegs in (("row", ns.cuda()), ("scalar", 37)):
        got = hb.elbo(xd, md, ld, *zd, nsegs, (B, T, F, strides, strides), False)
        torch.cuda.synchronize()
        for n, g in zip(NAMES, got):
            w = want[label][n]
            err = (g.detach().cpu().double() - w).abs()
            lim = 1e-5 + 1e-4 * w.abs()
            print("elbo_fwd B%d T%d F%d %s ns=%s %-11s worst share of the bound %.3f" % (B, T, F, "tm" if time_major else "bm", label, n,
                                                                                        (err / lim).max().item()))
            if not bool((err <= lim).all()):
                bad.append((label, n, err.max().item()))
    assert not bad, bad
