"""Writes tests/golden/tsne_whole_run.json: the final KL divergence and the 1-nearest-neighbour cluster purity of five float64
oracle runs of exact t-SNE (tests/tsne_ref.py) that differ in the seed of the initial map alone.  About 5 s per run on a CPU.

    python tests/golden/make_tsne_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import tsne_ref as R  # noqa: E402

N, D, CLUSTERS, CASE_SEED, PERPLEXITY, N_ITER = 300, 32, 6, 1, 30.0, 500


def main():
    X, label = R.make_case(N, D, CLUSTERS, CASE_SEED)
    d2 = R.sqdist(R.center(X))
    P = R.joint_p(d2, *R.affinity(d2, PERPLEXITY))
    kl, purity = [], []
    for seed in range(5):
        Y, _, _ = R.run(P, R.y0(N, seed), N_ITER, R.learning_rate(N), fast=True)
        kl.append(R.kl_divergence(P, Y))
        purity.append(R.purity_1nn(Y, label))
        print("seed %d: KL %.6f, purity %.4f" % (seed, kl[-1], purity[-1]))
    out = {"N": N, "D": D, "clusters": CLUSTERS, "case_seed": CASE_SEED, "perplexity": PERPLEXITY, "n_iter": N_ITER, "kl": kl,
           "purity": purity}
    with open(os.path.join(HERE, "tsne_whole_run.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
