"""The inference forward (fhvae_lstm_seq_infer / hip_binding.lstm_seq_infer) and the inference methods built on it (encode, decode,
reconstruct, convert, eval_model.py) on a MI355X.

  * bitwise equality with the training forward (hip_binding.lstm_seq) for every schedule, at the schedule the training forward takes
  * what it does not allocate (gates + c of a net) at the bench's model size
  * decode against the float64 CPU oracle; reconstruct against forward()'s log p(x|z) at zero noise; convert's identities
  * FHVAE_NO_INFER=1 parity; one eval_model.py run
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from lstm_lp_compare import make_inputs
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hb():
    import build_ext

    build_ext.build(verbose=False)
    import hip_binding

    hip_binding.load_library()
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return hip_binding


def _env(monkeypatch, env):
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)


# (B, T, I, Ic, H, L), dtype, env, top: the schedules and switches of test_lstm_lp_oracle_gpu.py
SEQ_CASES = [
    # per-step cells (bf16): the persistent kernels switched off; tiny / odd H; three layers
    ((256, 20, 80, 0, 256, 2), "bf16", {"FHVAE_NO_CLUSTER": "1"}, 2),
    ((5, 4, 8, 8, 8, 2), "bf16", {}, 2),
    ((33, 20, 80, 32, 48, 2), "bf16", {}, 0),
    ((256, 6, 80, 0, 256, 3), "bf16", {}, 1),
    # large-tile cells, bf16 and f32
    ((2048, 3, 80, 32, 512, 2), "bf16", {}, 2),
    ((2048, 3, 80, 32, 512, 2), "bf16", {}, 1),
    ((256, 4, 80, 32, 512, 2), "f32", {"FHVAE_BIG_CELLS": "1"}, 2),
    # contraction-split persistent form ("ks"): ragged B, I = 0, L = 1, H = 128
    ((256, 20, 80, 0, 256, 2), "bf16", {}, 2),
    ((100, 7, 80, 32, 256, 2), "bf16", {}, 0),
    ((16, 5, 0, 64, 256, 2), "bf16", {}, 1),
    ((64, 4, 80, 0, 256, 1), "bf16", {}, 2),
    ((300, 6, 40, 0, 128, 2), "bf16", {}, 0),
    # rows form with the 16-unit cluster forward (FHVAE_NO_FWD_WR=1), and at H = 128
    ((1024, 4, 80, 32, 256, 2), "bf16", {"FHVAE_NO_FWD_WR": "1"}, 2),
    ((1024, 4, 80, 32, 256, 2), "bf16", {"FHVAE_NO_FWD_WR": "1"}, 0),
    ((1500, 4, 80, 32, 128, 2), "bf16", {}, 1),
    # rows form with lstm_fwd_wr: T = 1, ragged clusters, more than one launch, I = 0, the decoder's top = 1
    ((2048, 20, 80, 0, 256, 2), "bf16", {}, 0),
    ((700, 1, 80, 0, 256, 2), "bf16", {}, 2),
    ((1100, 4, 80, 32, 256, 2), "bf16", {}, 2),
    ((4100, 2, 0, 64, 256, 1), "bf16", {}, 2),
    ((2048, 6, 0, 32, 256, 2), "bf16", {}, 1),
    # f32 per-step cells
    ((5, 4, 6, 0, 8, 2), "f32", {}, 2),
    ((7, 3, 0, 8, 16, 1), "f32", {}, 2),
    ((70, 20, 80, 0, 64, 2), "f32", {}, 2),
    ((300, 20, 80, 32, 256, 2), "f32", {}, 2),
    ((33, 1, 80, 32, 48, 2), "f32", {}, 0),
]


def _outputs(out, hn, top, bf):
    """The tensors a caller can read: hs_top (f32, top 2) or its bf16 twin (top 1), hn, hn_lp (top 0), the head shadows."""
    got = {"hn": hn}
    if getattr(hn, "_fh_lp", None) is not None:
        got["hn_lp"] = hn._fh_lp
    src = out if out is not None and out.dim() > 0 else hn
    if getattr(src, "_fh_head", None) is not None:
        got["head_wl"], got["head_wt"] = src._fh_head
    if out is not None and out.dim() > 0:
        if bf and top == 1:
            got["hs_lp"] = out._fh_lp
        else:
            got["hs_top"] = out
            if bf:
                got["hs_lp"] = out._fh_lp
    return got


@pytest.mark.parametrize("shape,dt,env,top", SEQ_CASES)
def test_infer_equals_training_forward_bitwise(hb, monkeypatch, shape, dt, env, top):
    _env(monkeypatch, env)
    B, T, I, Ic, H, L = shape
    bf = dt == "bf16"
    dtype = hb.BF16 if bf else hb.F32
    x, xc, params, _, _ = make_inputs(B, T, I, Ic, H, L, B + 7 * T + H + L)
    x = x.cuda() if x is not None else None
    xc = xc.cuda() if xc is not None else None
    params = [p.cuda() for p in params]
    head = None
    if bf and H % 8 == 0:  # a Gaussian head behind the net: its stacked bf16 operands ride in the operand-cast launch
        g = torch.Generator().manual_seed(B + H)
        K = H * L if top == 0 else H
        head = (torch.randn(16, K, generator=g).cuda(), torch.randn(16, K, generator=g).cuda())
    with torch.no_grad():
        want_out, want_hn = hb.lstm_seq(x, xc, T, params, dtype, top, head)
        want = _outputs(want_out, want_hn, top, bf)
        want_form = dict(hb.LAST_LSTM_FORM)
        got_out, got_hn = hb.lstm_seq_infer(x, xc, T, params, dtype, top, head)
        got = _outputs(got_out, got_hn, top, bf)
        got_form = dict(hb.LAST_LSTM_FORM)
    torch.cuda.synchronize()
    assert hb.lstm_sync_status() == 0
    assert got_form == want_form
    if bf and top == 0:
        assert got_out is None
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        assert torch.equal(got[k], want[k]), "%s differs (max |d| %g)" % (k, (got[k].float() - want[k].float()).abs().max())


def _c3(dt, B=2048):
    from fhvae import FHVAE

    torch.manual_seed(3)
    T, F, H, D = 20, 80, 256, 32
    m = FHVAE(T * F, [H, H], [H, H], D, D, [H, H], seg_len=T, num_seqs=100, compute_dtype=dt).cuda()
    return m, torch.randn(B, T, F, device="cuda")


def _peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base, out


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_encode_skips_gates_and_c(hb, monkeypatch, dt):
    m, x = _c3(dt)
    B, T, H, L = x.shape[0], x.shape[1], 256, 2
    es = 2 if dt == "bf16" else 4
    saved = L * T * B * 4 * H * es + L * T * B * H * 4  # gates + c of one net
    m.encode(x)  # warm-up (library, workspaces of the caching allocator)
    p_inf, a = _peak(lambda: m.encode(x))
    monkeypatch.setenv("FHVAE_NO_INFER", "1")
    p_ref, b = _peak(lambda: m.encode(x))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert p_ref - p_inf >= 0.9 * saved, (p_ref, p_inf, saved)
    assert hb.lstm_sync_status() == 0


def _close_elementwise(got, want, atol, rtol, what):
    got = got.detach().double().cpu()
    err = (got - want).abs()
    lim = atol + rtol * want.abs()
    assert bool((err <= lim).all()), "%s: worst excess %g" % (what, float((err - lim).max()))


@pytest.mark.parametrize("H,B", [(256, 96), (512, 64)])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_decode_vs_float64_oracle(hb, H, B, dt):
    from fhvae import FHVAE

    T, F, D = 20, 80, 32
    torch.manual_seed(H + B)
    ref = R.FHVAERef(T * F, [H, H], [H, H], D, D, [H, H], seg_len=T)
    m = FHVAE(T * F, [H, H], [H, H], D, D, [H, H], seg_len=T, compute_dtype=dt)
    m.load_state_dict(ref.state_dict(), strict=False)
    m.cuda()
    z1, z2 = torch.randn(B, D), torch.randn(B, D)
    with torch.no_grad():
        r64 = ref.double()
        out, _ = r64.pre_decoder.lstm(torch.cat([z1, z2], -1).double()[:, None, :].expand(B, T, -1))
        w_mu, w_lv = r64.dec_gauss_layer(out)
    g_mu, g_lv = m.decode(z1.cuda(), z2.cuda())
    assert g_mu.shape == (B, T, F) and g_lv.shape == (B, T, F) and g_mu.dtype == torch.float32
    if dt == "f32":
        _close_elementwise(g_mu, w_mu, 1e-5, 1e-4, "x_mu")
        _close_elementwise(g_lv, w_lv, 1e-5, 1e-4, "x_logvar")
    else:
        for g, w, n in ((g_mu, w_mu, "x_mu"), (g_lv, w_lv, "x_logvar")):
            _close_elementwise(g, w, 3e-2 * float(w.abs().max()), 0.0, n)
    # a broadcast z2 and wrong widths
    b_mu, _ = m.decode(z1.cuda(), z2[0].cuda())
    e_mu, _ = m.decode(z1.cuda(), z2[0].cuda().expand(B, D).contiguous())
    assert torch.equal(b_mu, e_mu)
    with pytest.raises(ValueError):
        m.decode(z1[:, :5].cuda(), z2.cuda())
    with pytest.raises(ValueError):
        m.decode(z1.cuda(), z2[:, :5].cuda())
    with pytest.raises(RuntimeError):
        m.decode(z1, z2)


def test_simple_fhvae_decode_vs_float64_oracle(hb):
    from simple_fhvae import SimpleFHVAE

    T, F, D, B = 20, 80, 32, 64
    torch.manual_seed(11)
    ref = R.SimpleFHVAERef(T * F, [128, 128], [128, 128], D, D, [128, 128])
    m = SimpleFHVAE(T * F, [128, 128], [128, 128], D, D, [128, 128])
    m.load_state_dict(ref.state_dict(), strict=False)
    m.cuda()
    z1, z2 = torch.randn(B, D), torch.randn(B, D)
    with torch.no_grad():
        r64 = ref.double()
        w_mu, w_lv = r64.dec_gauss_layer(r64.pre_decoder(torch.cat([z1, z2], -1).double()))
    g_mu, g_lv = m.decode(z1.cuda(), z2.cuda())
    assert g_mu.shape == (B, T * F)
    _close_elementwise(g_mu, w_mu, 1e-5, 1e-4, "x_mu")
    _close_elementwise(g_lv, w_lv, 1e-5, 1e-4, "x_logvar")
    x = torch.randn(B, T, F, device="cuda")
    r_mu, r_lv = m.reconstruct(x)
    assert r_mu.shape == x.shape and torch.equal(r_mu, m.decode(*m.encode(x))[0].reshape(x.shape))


def _log_px(x, mu, lv):
    x, mu, lv = (t.double().cpu() for t in (x, mu, lv))
    return (-0.5 * (np.log(2 * np.pi) + lv + (x - mu) ** 2 / lv.exp())).sum(dim=(1, 2))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_reconstruct_is_forward_decoder_at_zero_noise(hb, dt):
    from fhvae import FHVAE

    T, F, H, D, B, S = 20, 80, 256, 32, 256, 100
    torch.manual_seed(21)
    m = FHVAE(T * F, [H, H], [H, H], D, D, [H, H], seg_len=T, num_seqs=S, compute_dtype=dt).cuda()
    x = torch.randn(B, T, F, device="cuda")
    idx, ns = torch.randint(0, S, (B,)), torch.randint(3, 100, (B,))
    zero = (torch.zeros(B, D, device="cuda"), torch.zeros(B, D, device="cuda"))
    with torch.no_grad():
        lpx = m(x, idx, S, ns, eps=zero)[2].double().cpu()
    r_mu, r_lv = m.reconstruct(x)
    assert r_mu.shape == x.shape and r_lv.shape == x.shape
    got = _log_px(x, r_mu, r_lv)
    rtol = 1e-5 if dt == "f32" else 1e-2
    assert bool(((got - lpx).abs() <= rtol * lpx.abs()).all()), float(((got - lpx).abs() / lpx.abs()).max())


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_convert_identities(hb, dt):
    m, x = _c3(dt, B=300)
    z1, z2 = m.encode(x)
    y = m.mu2_table[7].detach()
    c_mu, c_lv = m.convert(x, y)
    d_mu, d_lv = m.decode(z1, y)
    assert torch.equal(c_mu, d_mu.reshape(x.shape)) and torch.equal(c_lv, d_lv.reshape(x.shape))
    e_mu, _ = m.convert(x, y.expand(x.shape[0], -1).contiguous())
    assert torch.equal(c_mu, e_mu)
    s_mu, s_lv = m.convert(x, z2)
    r_mu, r_lv = m.reconstruct(x)
    assert torch.equal(s_mu, r_mu) and torch.equal(s_lv, r_lv)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_no_infer_switch_parity(hb, monkeypatch, dt):
    m, x = _c3(dt, B=512)
    z = m.encode(x)
    d = m.decode(*z)
    r = m.reconstruct(x)
    monkeypatch.setenv("FHVAE_NO_INFER", "1")
    z_, d_, r_ = m.encode(x), m.decode(*z), m.reconstruct(x)
    for a, b in zip(z + d + r, z_ + d_ + r_):
        assert torch.equal(a, b)
    assert hb.lstm_sync_status() == 0


def test_eval_model_cli(hb, tmp_path):
    import utils
    from fhvae import FHVAE
    from train_model import synthetic_split

    T, F, H, D, S, N = 20, 16, 64, 16, 10, 40
    torch.manual_seed(5)
    m = FHVAE(T * F, [H, H], [H, H], D, D, [H, H], seg_len=T, num_seqs=S)
    utils.save_checkpoint(m, None, [], {}, "t", 1, 1, 0.0, 0.0, str(tmp_path))
    ck = str(tmp_path / "fhvae_t_e1.tar")
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "pytorch-scalablefhvae_amd", "eval_model.py"), "--checkpoint", ck, "--out", str(out),
           "--mels", str(F), "--num-seqs", str(S), "--segments", str(N), "--batch-size", "16", "--max-recon", "6", "--convert-to", "-1"]
    x, idx, _ = synthetic_split(N, T, F, S, 2)
    y = int(idx[0])
    cmd[-1] = str(y)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    z1, z2 = np.load(out / "z1_mu.npy"), np.load(out / "z2_mu.npy")
    assert z1.shape == (N, D) and z2.shape == (N, D)
    seqs = np.load(out / "mu2_seqs.npy")
    assert np.load(out / "mu2.npy").shape == (len(seqs), D) and set(seqs.tolist()) == set(idx.tolist())
    rx, rmu, rlv = np.load(out / "recon_x.npy"), np.load(out / "recon_mu.npy"), np.load(out / "recon_logvar.npy")
    assert rx.shape == rmu.shape == rlv.shape == (6, T, F)
    assert np.load(out / "convert_mu.npy").shape == (6, T, F)
    summary = json.load(open(out / "summary.json"))
    assert summary["segments"] == N and np.isfinite(summary["lower_bound_per_frame"])
    m = m.cuda()
    want_mu, want_lv = m.reconstruct(x[:6].cuda())
    assert np.array_equal(rx, x[:6].numpy())
    assert np.array_equal(rmu, want_mu.cpu().numpy()) and np.array_equal(rlv, want_lv.cpu().numpy())
