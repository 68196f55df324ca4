"""An ABX item file (abx.read_items' format) from TIMIT's phone transcriptions.

    python tools/timit_items.py RAW_DIR OUT.item [--sample-rate 16000] [--tier phn|wrd|phn-all]

Every .PHN / .phn file below RAW_DIR holds one `start_sample end_sample phone` line per phone, at 16 kHz.  Each phone becomes one
item: onset and offset in seconds, the phone, the phones in front of and behind it in the file as its context, the speaker (the
directory the file lies in, in lower case) and the utterance key `<speaker>_<name>` that preprocess_timit.py gives the .WAV next
to it.  The silence marker h# and the first and the last phone of a file (they have one neighbour only) are no tokens; h# may
be a context.  Files are walked in sorted order.  A malformed line is an error naming the file and the line.

With --tier wrd the .WRD / .wrd files are read instead (the same line format, a word in place of the phone): every word is one
item, the word stands in the #phone column as the term (qbe.queries_from_items) and both context columns hold `-`.

With --tier phn-all every phone of a .PHN file is a token, h# and the first and the last included; the context is `-` where a
neighbour is missing.  That is the transcription phone recognition is scored against (recognise_phones.py): an alignment without
those tokens would make every hypothesis phone over them an insertion.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pytorch-scalablefhvae_amd")]

SILENCE = "h#"


def read_phn(path):
    """-> [(start_sample, end_sample, phone)]"""
    rows = []
    with open(path) as fh:
        for no, line in enumerate(fh, 1):
            f = line.split()
            if not f:
                continue
            try:
                if len(f) != 3:
                    raise ValueError
                a, b = int(f[0]), int(f[1])
                if a < 0 or b < a:
                    raise ValueError
            except ValueError:
                raise ValueError("%s line %d: not `start_sample end_sample phone`: %r" % (path, no, line.rstrip("\n"))) from None
            rows.append((a, b, f[2]))
    return rows


def timit_items(raw_dir, sample_rate=16000, tier="phn"):
    """The items of every .PHN (tier "phn") or .WRD (tier "wrd") file below raw_dir, as abx.read_items returns them."""
    items = []
    exts = (".WRD", ".wrd") if tier == "wrd" else (".PHN", ".phn")
    for root, dirs, names in os.walk(raw_dir):
        dirs.sort()
        spk = os.path.basename(os.path.normpath(root)).lower()
        for name in sorted(names):
            stem, ext = os.path.splitext(name)
            if ext not in exts:
                continue
            rows = read_phn(os.path.join(root, name))
            if tier == "wrd":
                items += [("%s_%s" % (spk, stem), a / sample_rate, b / sample_rate, word, "-", "-", spk) for a, b, word in rows]
                continue
            if tier == "phn-all":
                items += [("%s_%s" % (spk, stem), a / sample_rate, b / sample_rate, phone, rows[k - 1][2] if k > 0 else "-",
                           rows[k + 1][2] if k + 1 < len(rows) else "-", spk) for k, (a, b, phone) in enumerate(rows)]
                continue
            for k in range(1, len(rows) - 1):
                a, b, phone = rows[k]
                if phone == SILENCE:
                    continue
                items.append(("%s_%s" % (spk, stem), a / sample_rate, b / sample_rate, phone, rows[k - 1][2], rows[k + 1][2], spk))
    return items


def main(argv=None):
    import abx

    ap = argparse.ArgumentParser(description="ABX item file from TIMIT's .PHN files")
    ap.add_argument("raw_dir")
    ap.add_argument("out_item")
    ap.add_argument("--sample-rate", type=int, default=16000)
    ap.add_argument("--tier", default="phn", choices=["phn", "wrd", "phn-all"],
                    help="phones with their contexts (ABX), words as search terms, or every phone of a file (the transcription for PER)")
    args = ap.parse_args(argv)
    try:
        items = timit_items(args.raw_dir, args.sample_rate, args.tier)
    except ValueError as e:
        print("timit_items: %s" % e, file=sys.stderr)
        return 1
    abx.write_items(args.out_item, items)
    print("%d items of %d utterances -> %s" % (len(items), len({it[0] for it in items}), args.out_item))
    return 0


if __name__ == "__main__":
    sys.exit(main())
