"""Build libfhvae_hip.so (gfx950) from csrc/*.hip with hipcc -- in-tree, no torch extension machinery.

    python pytorch-scalablefhvae_amd/build_ext.py [--force]

hipcc cross-compiles without a GPU.  The .so is git-ignored but travels to the GPU box.
"""
import concurrent.futures as cf
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(CSRC, "build")
LIB = os.path.join(HERE, "libfhvae_hip.so")
SOURCES = ["gemm.hip", "lstm.hip", "lstm_cluster.hip", "lstm_bwd_rs.hip", "lstm_fwd_wr.hip", "proj.hip", "loss.hip", "disc.hip", "disc_mfma.hip", "data.hip", "trace.hip", "wgrad.hip", "disc_lp.hip", "lstm_cell.hip", "hs.hip", "feats.hip", "synth.hip", "resample.hip", "melinv.hip", "kaldi_fbank.hip", "kaldi_cm.hip", "flac.hip", "sv.hip", "tsne.hip", "frames.hip", "vad.hip", "abx.hip", "kmeans.hip", "kaldi_post.hip", "qbe.hip", "gmm.hip", "probe.hip", "viterbi.hip", "ctc.hip", "falign.hip", "ctcbeam.hip", "segment.hip", "spk.hip", "ivector.hip", "snorm.hip"]
# -amdgpu-mfma-vgpr-form: MFMA results stay in VGPRs.  By default the backend puts accumulators in AGPRs and copies them
# around every non-MFMA use (v_accvgpr_read/write, 4 issue cycles each): 288 such moves in the long-K GEMM's loop, none with
# this form; measured 791 -> 810 k segments/s at B=2048, 275 -> 284 k at B=256.
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-fno-gpu-rdc", "-mllvm", "-amdgpu-mfma-vgpr-form"]
# per-file additions.  kaldi_cm.hip: its codecs must equal the host's bit for bit: every f32 operation rounded once (no fused
# multiply-add) and division correctly rounded
# sv.hip: its score is a correctly rounded division by correctly rounded square roots (the test's error bound rests on it)
# frames.hip: its windows and overlap means must equal the f32 expressions of include/fhvae_frames.h bit for bit, as kaldi_cm.hip
# vad.hip: its float64 sums are in the order include/fhvae_vad.h states and its one f32 product is rounded once, as frames.hip
# abx.hip: its f32 recursion and its float64 costs are the expressions of include/fhvae_abx.h, one rounding each, as frames.hip
# kmeans.hip: its scores, its f32 distance and its float64 sums are the expressions of include/fhvae_kmeans.h (no f32 division in it)
# kaldi_post.hip: its f32 chains are the explicit fmaf of include/fhvae_kaldi_post.h and nothing else is fused; its float64 sums,
# division and square root are the header's, one rounding each, as frames.hip
# qbe.hip: its f32 recursion and its float64 costs are the expressions of include/fhvae_qbe.h (the costs are abx.hip's), as abx.hip
# gmm.hip: its squares, its f32 sums and its float64 sums are the expressions of include/fhvae_gmm.h (no f32 division in it)
# probe.hip: its logits, its residuals and its float64 sums are the expressions of include/fhvae_probe.h, as gmm.hip
# viterbi.hip: its f32 additions are those of include/fhvae_viterbi.h, one rounding each (it holds no product; the flag keeps it so)
# ctc.hip: its float64 sums and differences are the expressions of include/fhvae_ctc.h as written, as probe.hip
# falign.hip: its float64 additions are those of include/fhvae_falign.h, one rounding each (it holds no product), as viterbi.hip
# ctcbeam.hip: its float64 sums and differences are the expressions of include/fhvae_ctcbeam.h as written, as ctc.hip
# segment.hip: its f32 scores are kmeans.hip's and its float64 sums and additions those of include/fhvae_segment.h, one rounding each
# spk.hip: its chains are the explicit fmaf of include/fhvae_spk.h, every other f32 operation is rounded once, and its one division
# and its square roots are correctly rounded (the row transform's length normalisation), as kaldi_post.hip
# ivector.hip: its f32 and float64 sums and its explicit fma chains are the expressions of include/fhvae_ivector.h, as gmm.hip
# snorm.hip: its f32 additions, its float64 sums and its one f32 division are the expressions of include/fhvae_snorm.h, one rounding
# each, as spk.hip (which holds the normalised score itself)
EXTRA_FLAGS = {"kaldi_cm.hip": ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"],
               "sv.hip": ["-fhip-fp32-correctly-rounded-divide-sqrt"],
               "frames.hip": ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"],
               "vad.hip": ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"],
               "abx.hip": ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"],
               "kmeans.hip": ["-ffp-contract=off"],
               "kaldi_post.hip": ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"],
               "qbe.hip": ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"],
               "gmm.hip": ["-ffp-contract=off"],
               "probe.hip": ["-ffp-contract=off"],
               "viterbi.hip": ["-ffp-contract=off"],
               "ctc.hip": ["-ffp-contract=off"],
               "falign.hip": ["-ffp-contract=off"],
               "ctcbeam.hip": ["-ffp-contract=off"],
               "segment.hip": ["-ffp-contract=off"],
               "spk.hip": ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"],
               "ivector.hip": ["-ffp-contract=off"],
               "snorm.hip": ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"]}


def _newer(a, b):
    return (not os.path.exists(b)) or os.path.getmtime(a) > os.path.getmtime(b)


def _deps():
    hdrs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    hdrs += [os.path.join(os.path.dirname(HERE), "include", h) for h in ("fhvae_hip.h", "fhvae_frames.h", "fhvae_vad.h", "fhvae_abx.h", "fhvae_kmeans.h", "fhvae_kaldi_post.h", "fhvae_qbe.h", "fhvae_gmm.h", "fhvae_probe.h", "fhvae_viterbi.h", "fhvae_ctc.h", "fhvae_falign.h", "fhvae_ctcbeam.h", "fhvae_segment.h", "fhvae_spk.h", "fhvae_ivector.h", "fhvae_snorm.h")]
    return hdrs


def build(force=False, verbose=True):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(OBJ, exist_ok=True)
    hdrs = _deps()
    jobs = []
    for s in SOURCES:
        src, obj = os.path.join(CSRC, s), os.path.join(OBJ, s.replace(".hip", ".o"))
        if force or _newer(src, obj) or any(_newer(h, obj) for h in hdrs):
            jobs.append((src, obj))

    def cc(job):
        src, obj = job
        cmd = [hipcc] + FLAGS + EXTRA_FLAGS.get(os.path.basename(src), []) + os.environ.get("FHVAE_EXTRA_HIPCC", "").split() + ["-c", src, "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed: %s\n%s" % (" ".join(cmd), r.stderr))
        return obj

    with cf.ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(cc, jobs))
    objs = [os.path.join(OBJ, s.replace(".hip", ".o")) for s in SOURCES]
    if jobs or force or not os.path.exists(LIB):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("link failed: %s\n%s" % (" ".join(cmd), r.stderr))
    if verbose:
        print("libfhvae_hip.so: %d translation unit(s) rebuilt -> %s" % (len(jobs), LIB))
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
