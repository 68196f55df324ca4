"""Speaker verification on the GPU: fhvae_sv_hist against the float64 oracle (tests/sv_ref.py), the edges of its definition,
determinism, the EER end to end and eval_model.py's options."""
import functools
import json

import numpy as np
import pytest
import torch

import sv_ref as R

pytestmark = pytest.mark.gpu

# (S, D, NB, speakers, seed)
CASES = [
    (321, 32, 1024, 12, 0),   # tails on both the 256 and the 64 tile
    (321, 16, 8192, 12, 1),   # the largest histogram
    (257, 64, 1024, 8, 2),    # one row past the stationary block
    (65, 32, 64, 5, 3),       # the smallest histogram
    (700, 32, 4096, 20, 4),   # several block pairs on and off the diagonal
]


@pytest.fixture(scope="module")
def hb():
    import build_ext

    build_ext.build(verbose=False)
    import hip_binding

    assert torch.cuda.is_available()
    return hip_binding


@functools.lru_cache(maxsize=None)
def oracle(case):
    """-> emb, label, and per class (row 0 targets, row 1 non-targets): scores, trials in bins >= k, trials within delta of edge k"""
    S, D, NB, speakers, seed = case
    emb, label = R.make_case(S, D, speakers, seed)
    emb.setflags(write=False), label.setflags(write=False)
    classes = []
    for s in R.trial_scores(emb, label):
        cum, near, _ = R.edge_counts(s, NB, R.delta(D))
        classes.append((s, cum, near))
    return emb, label, classes


def gpu_hist(hb, emb, label, NB):
    h = hb.sv_hist(torch.from_numpy(np.array(emb)).cuda(), torch.from_numpy(np.array(label)).cuda(), NB)  # (copies: views, read-only arrays)
    assert h.dtype == torch.int64 and tuple(h.shape) == (2, NB)
    return h.cpu().numpy()


def cum_ge(row):
    return np.concatenate([np.cumsum(row[::-1])[::-1], [0]])


def check_against_oracle(h, classes, what):
    for c, (s, cum, near) in enumerate(classes):
        assert int(h[c].sum()) == len(s), "%s: class %d holds %d trials, the oracle %d" % (what, c, h[c].sum(), len(s))
        diff = np.abs(cum_ge(h[c]) - cum)
        worst = int(np.argmax(diff - near))
        print("%s class %d: %d trials, largest |cum_gpu - cum_ref| %d, trials near an edge %d" % (what, c, len(s), diff.max(), near.sum()))
        assert (diff <= near).all(), "%s: class %d edge %d: |%d - %d| > %d trials within delta of it" % (
            what, c, worst, cum_ge(h[c])[worst], cum[worst], near[worst])


@pytest.mark.parametrize("case", CASES, ids=lambda c: "S%d-D%d-NB%d" % c[:3])
def test_histogram_against_oracle(hb, case):
    S, D, NB, _, _ = case
    emb, label, classes = oracle(case)
    # from the oracle alone: few trials sit within delta of an edge, so the tolerance cannot hide a wrong kernel
    every = np.concatenate([classes[0][0], classes[1][0]])
    share = R.near_share(every, NB, R.delta(D))
    print("share of trials within delta = %.3g of an edge: %.2f %%" % (R.delta(D), 100 * share))
    assert len(every) == S * (S - 1) // 2 and share <= 0.05
    check_against_oracle(gpu_hist(hb, emb, label, NB), classes, "S=%d D=%d NB=%d" % (S, D, NB))


def test_one_and_two_rows(hb):
    e = np.array([[1.0] * 16, [1.0] * 8 + [-1.0] * 8], dtype=np.float32)
    lab = np.array([4, 4], dtype=np.int32)
    assert not gpu_hist(hb, e[:1], lab[:1], 64).any()
    h = gpu_hist(hb, e, lab, 64)
    assert h.sum() == 1 and h[0, 32] == 1  # orthogonal rows of one speaker: a target trial of score 0
    h = gpu_hist(hb, e, np.array([4, 5], dtype=np.int32), 64)
    assert h.sum() == 1 and h[1, 32] == 1


@pytest.mark.parametrize("NB", [64, 8192])
def test_extreme_scores_and_zero_row(hb, NB):
    rs = np.random.RandomState(11)
    x = rs.randn(32).astype(np.float32)
    h = gpu_hist(hb, np.stack([x, x]), np.zeros(2, np.int32), NB)
    assert h.sum() == 1 and h[0, NB - 1] == 1
    h = gpu_hist(hb, np.stack([x, -x]), np.zeros(2, np.int32), NB)
    assert h.sum() == 1 and h[0, 0] == 1
    # a zero row scores 0 against everything, another zero row included
    e = np.concatenate([rs.randn(70, 32).astype(np.float32), np.zeros((2, 32), np.float32)])
    lab = np.arange(72, dtype=np.int32)
    h = gpu_hist(hb, e, lab, NB)
    assert h[0].sum() == 0 and h[1].sum() == 72 * 71 // 2
    rest = gpu_hist(hb, e[:70], lab[:70], NB)
    extra = h[1] - rest[1]
    assert extra[NB // 2] == 2 * 70 + 1 and extra.sum() == 2 * 70 + 1


def test_unlabelled_rows_take_part_in_no_trial(hb):
    case = CASES[0]
    emb, label, _ = oracle(case)
    lab = label.copy()
    drop = np.random.RandomState(5).rand(len(lab)) < 0.3
    drop[[0, 255, 256, 320]] = [True, False, True, True]
    lab[drop] = -1
    h = gpu_hist(hb, emb, lab, case[2])
    kept = gpu_hist(hb, emb[~drop], label[~drop], case[2])
    n = int((~drop).sum())
    assert h.sum() == n * (n - 1) // 2 and np.array_equal(h, kept)
    assert not gpu_hist(hb, emb, np.full(len(lab), -1, np.int32), case[2]).any()


def test_single_speaker_is_all_targets(hb):
    emb, _, _ = oracle(CASES[3])
    h = gpu_hist(hb, emb, np.full(len(emb), 3, np.int32), 64)
    assert h[1].sum() == 0 and h[0].sum() == len(emb) * (len(emb) - 1) // 2


def test_padding_to_a_multiple_of_16(hb):
    """D = 20 through the Python padding: zero columns add exact zeros, so the oracle's bound at D = 20 holds."""
    S, D, NB = 130, 20, 1024
    emb, label = R.make_case(S, D, 6, 9)
    classes = []
    for s in R.trial_scores(emb, label):
        cum, near, _ = R.edge_counts(s, NB, R.delta(D))
        classes.append((s, cum, near))
    check_against_oracle(gpu_hist(hb, emb, label, NB), classes, "D=20 padded")


def test_leading_dimension(hb):
    case = CASES[0]
    emb, label, _ = oracle(case)
    wide = torch.full((len(emb), 48), 7.0, device="cuda")
    wide[:, :32] = torch.from_numpy(np.array(emb)).cuda()
    view = wide[:, :32]
    assert view.stride(0) == 48 and not view.is_contiguous()
    h = hb.sv_hist(view, torch.from_numpy(np.array(label)).cuda(), case[2]).cpu().numpy()
    assert np.array_equal(h, gpu_hist(hb, emb, label, case[2]))
    # the C entry reads it in place
    lib = hb.load_library()
    lab = torch.from_numpy(np.array(label)).cuda()
    ws = torch.empty(int(lib.fhvae_sv_hist_ws_bytes(len(emb))), dtype=torch.uint8, device="cuda")
    out = torch.full((2, case[2]), -1, dtype=torch.int64, device="cuda")
    rc = lib.fhvae_sv_hist(view.data_ptr(), 48, lab.data_ptr(), len(emb), 32, case[2], ws.data_ptr(), ws.numel(), out.data_ptr(),
                           torch.cuda.current_stream().cuda_stream)
    assert rc == 0 and np.array_equal(out.cpu().numpy(), h)


@pytest.mark.parametrize("case", [CASES[0], CASES[4]], ids=lambda c: "S%d" % c[0])
def test_determinism_and_row_order(hb, case):
    emb, label, _ = oracle(case)
    NB = case[2]
    a, b = gpu_hist(hb, emb, label, NB), gpu_hist(hb, emb, label, NB)
    assert np.array_equal(a, b)
    # score(i, j) == score(j, i) bit for bit: which row of a trial is stationary does not move it to another bin
    perm = np.random.RandomState(case[4] + 100).permutation(len(emb))
    assert np.array_equal(gpu_hist(hb, emb[perm], label[perm], NB), a)
    assert np.array_equal(gpu_hist(hb, emb[::-1], label[::-1], NB), a)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "S%d-D%d-NB%d" % c[:3])
def test_eer_end_to_end(hb, case):
    import verification as V

    S, D, NB, _, _ = case
    emb, label, classes = oracle(case)
    (tar, cum_t, near_t), (non, cum_n, near_n) = classes
    exact = R.exact_eer(tar, non)
    # the oracle's own crossing bin k - 1, its mass, and the trials that may sit on the other side of its two edges
    frr, far = (len(tar) - cum_t) / len(tar), cum_n / len(non)
    k = int(np.argmax(frr >= far))
    ref = V.eer_from_hist(R.hist_ref(emb, label, NB))
    assert abs(ref["crossing_mass"] - ((frr[k] - frr[k - 1]) + (far[k - 1] - far[k]))) <= 1e-12
    bound = ref["crossing_mass"] + (near_t[k - 1] + near_t[k]) / len(tar) + (near_n[k - 1] + near_n[k]) / len(non)
    r = V.speaker_verification(emb, label, n_bins=NB)
    print("EER %.6f, exact %.6f, bound %.2e (crossing mass %.2e)" % (r["eer"], exact, bound, ref["crossing_mass"]))
    assert r["n_target"] == len(tar) and r["n_nontarget"] == len(non) and r["hist"].shape == (2, NB)
    assert abs(r["eer"] - exact) <= bound
    assert -1.0 <= r["threshold"] <= 1.0


def _speech_corpus(root, n_spk=3, n_utt=3, F=16):
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


def test_eval_model_cli(hb, tmp_path):
    import eval_model as EM
    import utils
    from fhvae import FHVAE

    T, F, H, D = 20, 16, 32, 16
    keys = _speech_corpus(tmp_path)
    n = len(keys)
    torch.manual_seed(5)
    m = FHVAE(T * F, [H, H], [H, H], D, D, [H, H], seg_len=T, num_seqs=n)
    utils.save_checkpoint(m, None, [], {}, "t", 1, 1, 0.0, 0.0, str(tmp_path))
    base = ["--checkpoint", str(tmp_path / "fhvae_t_e1.tar"), "--feat-scp", str(tmp_path / "feats.scp"), "--len-scp", str(tmp_path / "len.scp"),
            "--max-recon", "2"]

    plain, sv, u2s = tmp_path / "plain", tmp_path / "sv", tmp_path / "u2s"
    assert EM.main(base + ["--out", str(plain)]) == 0
    assert EM.main(base + ["--out", str(sv), "--spk-key-sep", "-", "--sv-bins", "256"]) == 0
    s_plain, s_sv = json.load(open(plain / "summary.json")), json.load(open(sv / "summary.json"))
    assert "speaker_verification" not in s_plain and not (plain / "sv_hist_mu2.npy").exists()
    block = s_sv.pop("speaker_verification")
    assert set(s_sv) == set(s_plain) and s_sv["segments"] == s_plain["segments"] and s_sv["sequences"] == s_plain["sequences"] == n
    assert np.array_equal(np.load(plain / "seq_ids.npy"), np.load(sv / "seq_ids.npy"))
    assert block["speakers"] == 3 and block["unlabelled"] == 0 and block["bins"] == 256
    assert set(block) == {"mu2", "z1_mean", "speakers", "unlabelled", "bins"}
    for name in ("mu2", "z1_mean"):
        b = block[name]
        assert set(b) == {"eer", "threshold", "n_target", "n_nontarget", "crossing_mass"}
        assert b["n_target"] + b["n_nontarget"] == n * (n - 1) // 2 and b["n_target"] == 3 * 3
        assert 0.0 <= b["eer"] <= 1.0
        h = np.load(sv / ("sv_hist_%s.npy" % name))
        assert h.shape == (2, 256) and h[0].sum() == b["n_target"] and h[1].sum() == b["n_nontarget"]
    # the histograms are those of the files the run wrote
    lab = np.repeat(np.arange(3, dtype=np.int32), 3)
    assert np.array_equal(np.load(sv / "sv_hist_mu2.npy"), gpu_hist(hb, np.load(sv / "mu2.npy"), lab, 256))

    # utt2spk with one sequence missing: it is unlabelled and takes part in no trial
    with open(tmp_path / "utt2spk", "w") as f:
        f.writelines("%s %s\n" % (k, k.split("-")[0]) for k in keys[1:])
    assert EM.main(base + ["--out", str(u2s), "--utt2spk", str(tmp_path / "utt2spk")]) == 0
    block = json.load(open(u2s / "summary.json"))["speaker_verification"]
    assert block["unlabelled"] == 1 and block["speakers"] == 3 and block["bins"] == 4096
    assert block["mu2"]["n_target"] + block["mu2"]["n_nontarget"] == (n - 1) * (n - 2) // 2
