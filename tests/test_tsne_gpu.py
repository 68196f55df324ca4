"""Exact t-SNE on the GPU (csrc/tsne.hip, tsne.py) against the float64 oracle (tests/tsne_ref.py).

Tolerances of the affinity, gradient, update and five-iteration checks are not fixed numbers: for every case the test measures
the error of the oracle run in float32 (expanded distances) against the oracle in float64 and allows the kernel FACTOR = 8
times that, with a floor of 1e-6 under the model's ratio (tsne_ref.tolerance).  Both figures are printed."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import tsne_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tsne_whole_run.json")

# (N, D, perplexity); the case's index is its seed and the number of clusters is 6 (case 0 has two duplicated rows)
CASES = [
    (321, 32, 30.0),  # tails on both the 256 and the 64 tile
    (257, 64, 10.0),  # one row past a stationary block
    (65, 16, 5.0),    # the smallest rows
    (130, 128, 8.0),  # the widest rows
    (700, 32, 30.0),  # several blocks and two chunks of the streamed range (512 + 188)
]
IDS = ["N%d-D%d-p%g" % c for c in CASES]


@pytest.fixture(scope="module")
def hb():
    import build_ext

    build_ext.build(verbose=False)
    import hip_binding

    assert torch.cuda.is_available()
    return hip_binding


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def oracle(case):
    """Everything the checks of one case share, computed once on the CPU: dict of read-only arrays."""
    N, D, perp = case
    X, label = R.make_case(N, D, 6, CASES.index(case))
    X = R.center(X)
    d64, d32 = R.sqdist(X), R.sqdist(X, np.float32)
    b64, m64, z64 = R.affinity(d64, perp)
    b32, m32, z32 = R.affinity(d32, perp)
    P64, P32 = R.joint_p(d64, b64, m64, z64), R.joint_p(d32, b32, m32, z32)
    lr = R.learning_rate(N)
    Y0 = R.y0(N, 0)
    s300 = tuple(a.astype(np.float32) for a in R.run(P64, Y0, 300, lr, fast=True))  # (what a float32 kernel can be handed)
    o = dict(X=X, label=label, d64=d64, b64=b64, b32=b32, m32=m32, z32=z32, P64=P64, P32=P32, lr=lr, Y0=Y0, Y300=s300[0], V300=s300[1],
             G300=s300[2])
    _frozen(*[v for v in o.values() if isinstance(v, np.ndarray)])
    return o


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: read-only arrays)


@functools.lru_cache(maxsize=None)
def gpu_affinity(case):
    import hip_binding as hb

    o = oracle(case)
    x = dev(o["X"])
    return (x,) + hb.tsne_affinity(x, case[2])


def report(what, got, model, ref, scalar=False):
    """Print and assert: the kernel's error ratio against the oracle within FACTOR times the float32 model's."""
    if scalar:
        e_k, e_m = abs(float(got) - float(ref)) / abs(float(ref)), abs(float(model) - float(ref)) / abs(float(ref))
    else:
        e_k, e_m = R.ratio(got, ref), R.ratio(model, ref)
    tol = R.tolerance(e_m)
    print("%-28s kernel %.2e   float32 model %.2e   allowed %.2e" % (what, e_k, e_m, tol))
    assert e_k <= tol, "%s: the kernel's error %.3e exceeds %.3e (float32 model: %.3e)" % (what, e_k, tol, e_m)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_affinities_have_the_perplexity(hb, case):
    N, D, perp = case
    o = oracle(case)
    _, beta, m, z = gpu_affinity(case)
    beta, m, z = (t.cpu().numpy() for t in (beta, m, z))
    assert beta.dtype == np.float32 and beta.shape == (N,) and np.isfinite(beta).all() and (beta > 0).all()
    d64 = o["d64"]
    report("perplexity", np.exp(R.entropy(d64, beta)) / perp, np.exp(R.entropy(d64, o["b32"])) / perp, np.ones(N))
    report("m", m, o["m32"], R.row_min(d64))
    # Z against the oracle evaluated at the kernel's beta; the model's Z against the oracle at the model's beta
    e_model = R.ratio(o["z32"], R.z_at(d64, o["b32"]))
    e_kernel = R.ratio(z, R.z_at(d64, beta))
    print("%-28s kernel %.2e   float32 model %.2e   allowed %.2e" % ("Z", e_kernel, e_model, R.tolerance(e_model)))
    assert e_kernel <= R.tolerance(e_model)
    if CASES.index(case) == 0:  # the duplicated rows: the nearest row is at distance exactly 0
        assert m[3] == 0.0 and m[N // 2] == 0.0


def _gradient_check(hb, case, Y, a, what):
    o = oracle(case)
    x, beta, m, z = gpu_affinity(case)
    out, scal = hb.tsne_grad(x, beta, m, z, dev(Y), a)
    out, scal = out.cpu().numpy(), scal.cpu().numpy()
    ref = R.gradient(o["P64"], np.asarray(Y, dtype=np.float64), a)
    mod = R.gradient(o["P32"], np.asarray(Y, dtype=np.float32), a)
    print("%s, N = %d, D = %d, exaggeration %g" % (what, case[0], case[1], a))
    report("F", out[:, 0:2], mod["F"], ref["F"])
    report("R", out[:, 2:4], mod["R"], ref["R"])
    report("W", out[:, 4], mod["W"], ref["W"])
    report("grad", out[:, 5:7], mod["grad"], ref["grad"])
    report("Zq", scal[0], mod["Zq"], ref["Zq"], scalar=True)
    report("KL", scal[1], mod["kl"], ref["kl"], scalar=True)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gradient_at_the_initial_map(hb, case):
    _gradient_check(hb, case, oracle(case)["Y0"], 12.0, "Y0")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gradient_after_300_iterations(hb, case):
    _gradient_check(hb, case, oracle(case)["Y300"], 1.0, "the oracle's state after 300 iterations")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_one_update_after_300_iterations(hb, case):
    o = oracle(case)
    x, beta, m, z = gpu_affinity(case)
    a, mom = R.schedule(300)
    Y, V, G = o["Y300"], o["V300"], o["G300"]
    ref_grad = R.gradient(o["P64"], Y.astype(np.float64), a)["grad"]
    ref = R.update(Y.astype(np.float64), V.astype(np.float64), G.astype(np.float64), ref_grad, mom, o["lr"])
    mod_grad = R.gradient(o["P32"], Y, a)["grad"]
    mod = R.update(Y.copy(), V.copy(), G.copy(), mod_grad, mom, np.float32(o["lr"]))
    # where the gradient is next to nothing the sign test of the gains can flip: from the oracle alone, a few elements
    keep = np.abs(ref_grad) >= 1e-4 * np.abs(ref_grad).max()
    print("elements left out (|grad| below 1e-4 of its maximum): %d of %d" % ((~keep).sum(), keep.size))
    assert (~keep).mean() <= 0.02
    y, v, g = dev(Y), dev(V), dev(G)
    hb.tsne_step(x, beta, m, z, y, v, g, a, mom, o["lr"])
    for name, got, mo, re in (("G", g, mod[2], ref[2]), ("V", v, mod[1], ref[1]), ("Y", y, mod[0], ref[0])):
        report(name, got.cpu().numpy()[keep], mo[keep], re[keep])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_five_iterations_from_the_initial_map(hb, case):
    o = oracle(case)
    x, beta, m, z = gpu_affinity(case)
    ref = R.run(o["P64"], o["Y0"], 5, o["lr"])[0]
    mod = R.run(o["P32"], o["Y0"], 5, np.float32(o["lr"]))[0]
    y = dev(o["Y0"])
    v, g = torch.zeros_like(y), torch.ones_like(y)
    ws = hb.tsne_workspace(x)
    for it in range(5):
        a, mom = R.schedule(it)
        hb.tsne_step(x, beta, m, z, y, v, g, a, mom, o["lr"], ws=ws)
    report("Y after 5 iterations", y.cpu().numpy(), mod, ref)


def test_whole_run(hb):
    """500 iterations at N = 300: the final KL, recomputed in float64 from the returned map, is no worse than the worst of five
    float64 oracle runs (initial maps of seeds 0..4, tests/golden/tsne_whole_run.json, made by tests/golden/make_tsne_golden.py)
    plus their spread; the map's 1-nearest-neighbour cluster purity equals the oracle's."""
    import tsne as T

    gold = json.load(open(GOLDEN))
    N, D, perp, iters = gold["N"], gold["D"], gold["perplexity"], gold["n_iter"]
    X, label = R.make_case(N, D, gold["clusters"], gold["case_seed"])
    Y, info = T.tsne(X, perplexity=perp, n_iter=iters, seed=0)
    assert Y.shape == (N, 2) and Y.dtype == np.float32 and np.isfinite(Y).all()
    assert info["perplexity"] == perp and info["n_iter"] == iters and info["seed"] == 0
    d64 = R.sqdist(R.center(X))
    P = R.joint_p(d64, *R.affinity(d64, perp))
    kl = R.kl_divergence(P, Y)
    bound = max(gold["kl"]) + (max(gold["kl"]) - min(gold["kl"]))
    purity = R.purity_1nn(Y, label)
    print("oracle KL of seeds 0..4: %s; bound %.6f" % (" ".join("%.6f" % k for k in gold["kl"]), bound))
    print("kernel: KL of the returned map %.6f (float64), reported by the last step %.6f, purity %.4f (oracle %s)"
          % (kl, info["kl"], purity, gold["purity"]))
    assert kl <= bound
    assert purity == gold["purity"][0] and all(p == gold["purity"][0] for p in gold["purity"])
    assert abs(info["kl"] - kl) <= 0.01 * kl  # (the step's figure is that of the map before its last update)


@pytest.mark.parametrize("case", [CASES[0], CASES[4]], ids=[IDS[0], IDS[4]])
def test_determinism(hb, case):
    o = oracle(case)

    def once():
        x = dev(o["X"])
        beta, m, z = hb.tsne_affinity(x, case[2])
        y = dev(o["Y0"])
        v, g = torch.zeros_like(y), torch.ones_like(y)
        kl = torch.zeros(1, device="cuda")
        for it in range(20):
            hb.tsne_step(x, beta, m, z, y, v, g, 12.0, 0.5, o["lr"], kl=kl if it == 19 else None)
        return [t.cpu().numpy() for t in (beta, m, z, y, v, g, kl)]

    for a, b in zip(once(), once()):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("case", [CASES[0], CASES[3]], ids=[IDS[0], IDS[3]])
def test_leading_dimension(hb, case):
    N, D, perp = case
    o = oracle(case)
    x, beta, m, z = gpu_affinity(case)
    wide = torch.full((N, D + 4), 7.0, device="cuda")
    wide[:, :D] = x
    view = wide[:, :D]
    assert view.stride(0) == D + 4 and not view.is_contiguous()
    got = hb.tsne_affinity(view, perp)
    for a, b in zip(got, (beta, m, z)):
        assert torch.equal(a, b)
    y = dev(o["Y300"])
    (out_v, scal_v), (out_p, scal_p) = hb.tsne_grad(view, beta, m, z, y, 1.0), hb.tsne_grad(x, beta, m, z, y, 1.0)
    assert torch.equal(out_v, out_p) and torch.equal(scal_v, scal_p)
    # the C entry reads the rows in place
    lib = hb.load_library()
    ws = hb.tsne_workspace(x)
    b2 = torch.empty_like(beta)
    rc = lib.fhvae_tsne_affinity(view.data_ptr(), D + 4, N, D, perp, b2.data_ptr(), torch.empty_like(m).data_ptr(),
                                 torch.empty_like(z).data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0 and torch.equal(b2, beta)


def test_padding_to_a_multiple_of_16(hb):
    """D = 20 through the Python padding: zero columns change no distance."""
    X, _ = R.make_case(90, 20, 4, 7)
    X = R.center(X)
    d64 = R.sqdist(X)
    beta = hb.tsne_affinity(dev(X), 6.0)[0].cpu().numpy()
    b32 = R.affinity(R.sqdist(X, np.float32), 6.0)[0]
    report("perplexity, D = 20", np.exp(R.entropy(d64, beta)) / 6.0, np.exp(R.entropy(d64, b32)) / 6.0, np.ones(90))


def _speech_corpus(root, n_spk=4, n_utt=4, F=16):
    rs = np.random.RandomState(3)
    keys = []
    with open(root / "feats.scp", "w") as fs, open(root / "len.scp", "w") as ls:
        for s in range(n_spk):
            for u in range(n_utt):
                key, n = "s%02d-1-%04d" % (s + 1, u + 7), 36 + 8 * ((s + u) % 3)
                np.save(root / (key + ".npy"), (rs.randn(n, F) + s).astype(np.float32))
                fs.write("%s %s\n" % (key, root / (key + ".npy")))
                ls.write("%s %d\n" % (key, n))
                keys.append(key)
    return keys


TSNE_FILES = ("tsne_mu2.npy", "tsne_z1_mean.npy", "tsne.tsv", "tsne_mu2.png", "tsne_z1_mean.png")


@pytest.fixture(scope="module")
def eval_runs(hb, tmp_path_factory):
    """eval_model.py on a tiny generated corpus: without --tsne, with it, and with it and the speakers."""
    import eval_model as EM
    import utils
    from fhvae import FHVAE

    tmp = tmp_path_factory.mktemp("tsne_eval")
    T, F, H, D = 20, 16, 32, 16
    keys = _speech_corpus(tmp)
    torch.manual_seed(5)
    m = FHVAE(T * F, [H, H], [H, H], D, D, [H, H], seg_len=T, num_seqs=len(keys))
    utils.save_checkpoint(m, None, [], {}, "t", 1, 1, 0.0, 0.0, str(tmp))
    base = ["--checkpoint", str(tmp / "fhvae_t_e1.tar"), "--feat-scp", str(tmp / "feats.scp"), "--len-scp", str(tmp / "len.scp"),
            "--max-recon", "2"]
    opts = ["--tsne", "--tsne-perplexity", "4", "--tsne-iters", "40", "--tsne-seed", "3"]
    assert EM.main(base + ["--out", str(tmp / "plain")]) == 0
    assert EM.main(base + ["--out", str(tmp / "maps")] + opts) == 0
    assert EM.main(base + ["--out", str(tmp / "spk"), "--spk-key-sep", "-"] + opts) == 0
    return tmp, keys, base


def test_eval_model_tsne(hb, eval_runs):
    import eval_model as EM

    tmp, keys, base = eval_runs
    n = len(keys)
    s_plain = json.load(open(tmp / "plain" / "summary.json"))
    assert "tsne" not in s_plain and not any((tmp / "plain" / f).exists() for f in TSNE_FILES)
    for run in ("maps", "spk"):
        out = tmp / run
        s = json.load(open(out / "summary.json"))
        block = s.pop("tsne")
        s.pop("speaker_verification", None)
        assert set(s) == set(s_plain) and s["segments"] == s_plain["segments"] and s["sequences"] == n
        assert set(block) == {"perplexity", "iterations", "seed", "kl_mu2", "kl_z1_mean"}
        assert block["perplexity"] == 4.0 and block["iterations"] == 40 and block["seed"] == 3
        assert np.isfinite(block["kl_mu2"]) and np.isfinite(block["kl_z1_mean"]) and block["kl_mu2"] > 0
        for name in ("mu2", "z1_mean"):
            y = np.load(out / ("tsne_%s.npy" % name))
            assert y.shape == (n, 2) and y.dtype == np.float32 and np.isfinite(y).all()
        lines = [l.rstrip("\n").split("\t") for l in open(out / "tsne.tsv")]
        assert [l[0] for l in lines] == keys and all(len(l) == 6 for l in lines)
        assert [l[1] for l in lines] == ([k.split("-")[0] for k in keys] if run == "spk" else ["-"] * n)
        assert np.allclose(np.array([[float(v) for v in l[2:4]] for l in lines]), np.load(out / "tsne_mu2.npy"), rtol=1e-5, atol=0)
        assert np.load(out / "mu2.npy").shape == np.load(tmp / "plain" / "mu2.npy").shape
    # the map is that of the file the run wrote
    import tsne as T

    again, _ = T.tsne(np.load(tmp / "maps" / "mu2.npy"), perplexity=4.0, n_iter=40, seed=3)
    assert np.array_equal(again, np.load(tmp / "maps" / "tsne_mu2.npy"))
    assert not (tmp / "maps" / "tsne_mu2.png").exists()  # (no speakers: nothing to colour by)
    # a perplexity too large for the sequences is an error that names both
    assert EM.main(base + ["--out", str(tmp / "bad"), "--tsne", "--tsne-perplexity", "30"]) == 1


def test_eval_model_tsne_pictures(hb, eval_runs):
    pytest.importorskip("matplotlib")
    tmp = eval_runs[0]
    for name in ("tsne_mu2.png", "tsne_z1_mean.png"):
        data = open(tmp / "spk" / name, "rb").read()
        assert data[:8] == b"\x89PNG\r\n\x1a\n" and len(data) > 2000
