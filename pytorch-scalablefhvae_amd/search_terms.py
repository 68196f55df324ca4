"""search_terms.py -- query-by-example search of a whole corpus: where do the spoken examples of an item file occur?  Every query
is aligned against every utterance by subsequence DTW on the frame-level z1 of a trained checkpoint (or on the input features,
the baseline); qbe.py does the work ("Query by example").

    python pytorch-scalablefhvae_amd/search_terms.py --checkpoint CK --feat-scp S --len-scp S [--data-format numpy|kaldi]
        [--mvn-path P] --queries ITEM --out DIR [--on z1|feats] [--query-feat-scp S --query-len-scp S] [--item ITEM]
        [--distance angular|cosine] [--frame-shift 0.010] [--frame-offset 0.0] [--max-per-term 5] [--top 10]
        [--batch-size B] [--compute-dtype f32|bf16]

  --queries ITEM     the examples (abx.read_items' format; the #phone column is the term, tools/timit_items.py --tier wrd writes
                     one): tokens of at most 64 frames, the first --max-per-term of every term (0: all)
  --query-feat-scp   the corpus the queries are cut from, when it is not the searched one (with --query-len-scp; the same
                     --data-format and --mvn-path).  By default they are cut from the searched corpus, and a query's own
                     utterance is then no candidate for it
  --item ITEM        the term tokens of the searched corpus: MAP, P@N, P@10 and the share of located tokens (qbe.rank_metrics)

It writes under --out: hits.tsv (query id, term, rank, utterance key, start s, end s, cost: the --top best utterances per query)
and qbe.json: on, queries, dropped, distance, utterances, frames and, with --item, map, p_at_n, p_at_10, located, no_target.
"""
from __future__ import annotations

import argparse
import json
import os
import sys


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Query-by-example search: subsequence DTW on frame-level latents, on the GPU")
    p.add_argument("--checkpoint", required=True)
    p.add_argument("--feat-scp", required=True)
    p.add_argument("--len-scp", required=True)
    p.add_argument("--data-format", default="numpy", choices=["numpy", "kaldi"], help="what --feat-scp points at")
    p.add_argument("--mvn-path", default=None)
    p.add_argument("--out", required=True, help="output directory (created)")
    p.add_argument("--on", default="z1", choices=["z1", "feats"], help="frame-level z1, or the normalised input features")
    p.add_argument("--queries", required=True, metavar="ITEM", help="the examples to search for")
    p.add_argument("--query-feat-scp", default=None, metavar="S", help="the corpus the queries are cut from (default: the searched one)")
    p.add_argument("--query-len-scp", default=None, metavar="S")
    p.add_argument("--item", default=None, metavar="ITEM", help="the term tokens of the searched corpus, to score the ranking against")
    p.add_argument("--distance", default="angular", choices=["angular", "cosine"], help="frame cost under the DTW")
    p.add_argument("--frame-shift", type=float, default=0.010, help="seconds between frames")
    p.add_argument("--frame-offset", type=float, default=0.0, help="time of frame 0 in seconds")
    p.add_argument("--max-per-term", type=int, default=5, help="queries kept per term, the first in file order; 0: all")
    p.add_argument("--top", type=int, default=10, help="utterances listed per query in hits.tsv")
    p.add_argument("--batch-size", type=int, default=16384, help="windows per forward")
    p.add_argument("--compute-dtype", default=None, choices=["f32", "bf16"], help="default: the checkpoint's")
    return p


def parse_args(argv=None):
    p = build_parser()
    args = p.parse_args(argv)
    if (args.query_feat_scp is None) != (args.query_len_scp is None):
        p.error("--query-feat-scp and --query-len-scp come together")
    if not args.frame_shift > 0:
        p.error("--frame-shift %g must be positive" % args.frame_shift)
    if args.max_per_term < 0 or args.top < 1 or args.batch_size < 1:
        p.error("--max-per-term must not be negative, --top and --batch-size must be at least 1")
    return p, args


def main(argv=None) -> int:
    parser, args = parse_args(argv)
    import torch

    import utils

    model = utils.load_checkpoint_file(args.checkpoint, finetune=True)[0].eval()
    T = int(getattr(model, "seg_len", 20))
    if args.compute_dtype is not None:
        if not hasattr(model, "compute_dtype"):
            parser.error("--compute-dtype: a %s checkpoint computes in f32 only" % model.model)
        model.compute_dtype = args.compute_dtype
    if not torch.cuda.is_available():
        print("the search runs on a MI355X only (no CPU fallback)", file=sys.stderr)
        return 1
    import abx
    import frames
    import hip_binding as hb
    import qbe

    dev = torch.device("cuda:0")
    model = model.to(dev)
    same = args.query_feat_scp is None
    try:
        pool = frames.pool_from_scp(args.data_format, args.feat_scp, args.len_scp, args.mvn_path, T, 1, dev)
        rows = qbe.corpus_rows(model, pool, args.on, args.batch_size)
        qpool = pool if same else frames.pool_from_scp(args.data_format, args.query_feat_scp, args.query_len_scp, args.mvn_path, T, 1, dev)
        qrows = rows if same else qbe.corpus_rows(model, qpool, args.on, args.batch_size)
        queries = qbe.queries_from_items(abx.read_items(args.queries), qpool.keys, qpool.lengths, args.frame_shift, args.frame_offset,
                                         max_per_term=args.max_per_term)
        grid = qbe.search(qrows, queries, rows, qbe.utt_ptr_of(pool.lengths), args.distance)
        info = {"on": args.on, "queries": len(queries["id"]), "dropped": queries["dropped"], "distance": args.distance,
                "utterances": len(pool.keys), "frames": int(rows.shape[0])}
        if args.item is not None:
            truth = qbe.truth_from_items(abx.read_items(args.item), pool.keys, pool.lengths, args.frame_shift, args.frame_offset)
            res = qbe.rank_metrics(grid["best_cost"], grid["best_start"], grid["best_end"], queries, truth, same)
            info.update({k: res[k] for k in ("map", "p_at_n", "p_at_10", "located", "no_target")})
    except (ValueError, OSError) as e:
        print("search_terms: %s" % e, file=sys.stderr)
        return 1
    if hb.lstm_sync_status() != 0:
        print("a persistent recurrence launch gave up: the results are invalid", file=sys.stderr)
        return 3
    os.makedirs(args.out, exist_ok=True)
    hits = qbe.top_hits(grid["best_cost"], grid["best_start"], grid["best_end"], queries, args.top, same)
    qbe.write_hits(os.path.join(args.out, "hits.tsv"), hits, queries, pool.keys, args.frame_shift, args.frame_offset)
    with open(os.path.join(args.out, "qbe.json"), "w") as f:
        json.dump(info, f, indent=1)
    print(json.dumps(info))
    return 0


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.exit(main())
