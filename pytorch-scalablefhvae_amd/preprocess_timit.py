"""preprocess_timit.py -- wav.scp files for the train / dev / test sets of a TIMIT copy (the reference's preprocess_timit.py).

    python pytorch-scalablefhvae_amd/preprocess_timit.py RAW_DATA_DIR OUTPUT_DIR --dev_spk DEV_SPEAKERS --test_spk TEST_SPEAKERS

Every file below RAW_DATA_DIR whose name ends in .wav or .WAV becomes one "<speaker>_<name> <path>" line, the speaker being
the directory the file lies in, in lower case.  A speaker named in DEV_SPEAKERS (one per line) goes to OUTPUT_DIR/dev/wav.scp,
one in TEST_SPEAKERS to test/wav.scp, everyone else to train/wav.scp; each list is sorted by utterance id.

Differences from the reference:
  * TIMIT's .WAV files are NIST SPHERE files, and wav.scp lists them where they are: features.read_audio reads SPHERE, so no
    converted copy is written to OUTPUT_DIR/wav (the reference converted every file with sphfile).
  * the two speaker lists are required arguments: the defaults the reference names (misc/timit_dev_spk.list,
    misc/timit_test_spk.list) are not among its files.
"""
from __future__ import annotations

import argparse
import os
import sys
from pathlib import Path

SET_NAMES = ("train", "dev", "test")


def read_speakers(path):
    with open(path) as fh:
        return {line.strip().lower() for line in fh if line.strip()}


def process_timit(raw_data_dir, output_dir, dev_spk_path, test_spk_path):
    """Writes <output_dir>/{train,dev,test}/wav.scp; returns the three paths."""
    dev, test = read_speakers(dev_spk_path), read_speakers(test_spk_path)
    both = sorted(dev & test)
    if both:
        raise ValueError("speaker(s) %s are in both %s and %s" % (", ".join(both), dev_spk_path, test_spk_path))
    entries = {name: [] for name in SET_NAMES}
    for root, _, names in os.walk(raw_data_dir):
        spk = os.path.basename(os.path.normpath(root)).lower()
        which = "dev" if spk in dev else "test" if spk in test else "train"
        for name in names:
            if name.endswith(".wav") or name.endswith(".WAV"):
                entries[which].append((f"{spk}_{os.path.splitext(name)[0]}", os.path.join(root, name)))
    paths = []
    for name in SET_NAMES:
        scp = Path(output_dir) / name / "wav.scp"
        os.makedirs(scp.parent, exist_ok=True)
        with open(scp, "w") as fh:
            for uid, path in sorted(entries[name]):
                fh.write(f"{uid} {path}\n")
        print(f"{name}: {len(entries[name])} utterances -> {scp}")
        paths.append(scp)
    print("Dumped .scp files")
    return tuple(paths)


def build_parser():
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("raw_data_dir", type=str, help="TIMIT raw data directory")
    p.add_argument("output_dir", type=str, help="Directory for data output")
    p.add_argument("--dev_spk", type=str, required=True, help="Path to list of dev set speakers")
    p.add_argument("--test_spk", type=str, required=True, help="Path to list of test set speakers")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    print(args)
    process_timit(args.raw_data_dir, args.output_dir, args.dev_spk, args.test_spk)
    return 0


if __name__ == "__main__":
    sys.exit(main())
