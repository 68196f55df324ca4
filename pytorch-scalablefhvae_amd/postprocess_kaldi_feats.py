"""postprocess_kaldi_feats.py -- delta features and sliding-window CMVN of any Kaldi feature archive, on the MI355X
(add-deltas and apply-cmvn-sliding; kaldi_post.add_deltas / cmvn_sliding, no Kaldi binary is run).

    python pytorch-scalablefhvae_amd/postprocess_kaldi_feats.py --feat-scp IN/feats.scp --len-scp IN/len.scp --out DIR
        [--add-deltas [--delta-order 2] [--delta-window 2]]
        [--cmvn-sliding [--cmn-window 300] [--cmn-min-window 100] [--no-cmn-center] [--cmn-norm-vars]]
        [--compress [--compression-method auto]]

Reads every matrix feats.scp names (float or compressed; the z1 archive extract_latents.py writes is the intended input),
checks its row count against len.scp, applies the deltas and then the CMVN, each utterance on its own, and writes
DIR/feats.ark, DIR/feats.scp and DIR/len.scp in the input's order, which datasets.KaldiDataset reads back.  At least one of
--add-deltas and --cmvn-sliding is needed.
"""
from __future__ import annotations

import argparse
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import kaldi_io_lite  # noqa: E402
import prepare_kaldi_data  # noqa: E402

BATCH_UTTS = 512  # utterances read ahead of a device batch


def read_scp(path, what):
    out = []
    with open(path) as fh:
        for ln, line in enumerate(fh, 1):
            if not line.strip():
                continue
            parts = line.rstrip().split(None, 1)
            if len(parts) != 2:
                raise ValueError("%s:%d: expected \"<key> <%s>\"" % (path, ln, what))
            out.append((parts[0], parts[1]))
    return out


def postprocess(feat_scp, len_scp, out_dir, deltas=None, cmvn=None, compress=None):
    """-> (count, (feats.ark, feats.scp, len.scp)).  `deltas` / `cmvn`: kaldi_post.deltas_spec / cmvn_spec."""
    import kaldi_post

    if deltas is None and cmvn is None:
        raise ValueError("nothing to do: pass --add-deltas and / or --cmvn-sliding")
    entries = read_scp(feat_scp, "archive:offset")
    lens = dict(read_scp(len_scp, "nframes"))
    for key, _ in entries:
        if key not in lens:
            raise ValueError("%s: %s has no entry" % (len_scp, key))
    os.makedirs(out_dir, exist_ok=True)
    ark, scp, lscp = (os.path.join(out_dir, n) for n in ("feats.ark", "feats.scp", "len.scp"))
    written = []

    def items():
        for i in range(0, len(entries), BATCH_UTTS):
            chunk = entries[i:i + BATCH_UTTS]
            mats = []
            for key, spec in chunk:
                m = kaldi_io_lite.load_mat(spec)
                if len(m) != int(lens[key]):
                    raise ValueError("%s: %d rows in %s, %s in %s" % (key, len(m), feat_scp, lens[key], len_scp))
                mats.append(m)
            got = kaldi_post.post_process(mats, deltas, cmvn, compress=compress, names=[k for k, _ in chunk])
            for (key, _), m in zip(chunk, got):
                written.append((key, len(m)))
                yield key, m

    count = kaldi_io_lite.write_ark_scp(ark, scp, items())
    kaldi_io_lite.write_len_scp(lscp, written)
    return count, (ark, scp, lscp)


def build_parser():
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--feat-scp", type=str, required=True, help="feats.scp of the input archive")
    p.add_argument("--len-scp", type=str, required=True, help="len.scp of the input archive")
    p.add_argument("--out", type=str, required=True, help="Directory that receives feats.ark, feats.scp and len.scp")
    prepare_kaldi_data.add_post_arguments(p)
    p.add_argument("--compress", action="store_true", help="Write Kaldi compressed matrices (coded on the GPU), as copy-feats --compress=true does")
    p.add_argument("--compression-method", type=str, default="auto", choices=list(kaldi_io_lite.METHODS),
                   help="With --compress: Kaldi's automatic method, or two or one byte per value")
    return p


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    deltas, cmvn = prepare_kaldi_data.post_specs(parser, args)
    if deltas is None and cmvn is None:
        parser.error("nothing to do: pass --add-deltas and / or --cmvn-sliding")
    if os.path.abspath(args.out) == os.path.abspath(os.path.dirname(args.feat_scp) or "."):
        parser.error("--out is the directory of --feat-scp: the input archive would be overwritten")
    print(args)
    try:
        count, _ = postprocess(args.feat_scp, args.len_scp, args.out, deltas, cmvn, args.compression_method if args.compress else None)
    except ValueError as e:
        print("postprocess_kaldi_feats: %s" % e, file=sys.stderr)
        return 1
    print("Processed %d matrices into %s." % (count, args.out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
