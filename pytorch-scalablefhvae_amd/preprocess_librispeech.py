"""preprocess_librispeech.py -- wav.scp files for the train / dev / test sets of a LibriSpeech download (the reference's
preprocess_librispeech.py, same command line).

    python pytorch-scalablefhvae_amd/preprocess_librispeech.py RAW_DATA_DIR OUTPUT_DIR [--data-format {numpy,kaldi}]
        [--train_list train-clean-100 ...] [--dev_list dev-clean dev-other] [--test_list test-clean test-other]

RAW_DATA_DIR holds the subsets as LibriSpeech unpacks them (train-clean-100/<speaker>/<chapter>/<utterance>.flac).  Every
.flac file below the listed subsets that exist becomes one "<utterance id> <path>" line of OUTPUT_DIR/<set>/wav.scp, the
utterance id being the file name without its extension, sorted by utterance id.

Differences from the reference:
  * wav.scp lists the .flac files themselves for both data formats: prepare_numpy_data.py and prepare_kaldi_data.py decode
    FLAC on the GPU (features.read_audio_batch), so nothing is converted to WAV for Kaldi (the reference ran pydub / ffmpeg
    over every file) and --data-format changes nothing here; it is kept for the command line.
  * the test list of process_librispeech() defaults to test-clean test-other like the command line (the reference's function
    default repeats dev-other).
  * an utterance is listed once, and a set is sorted as a whole (the reference writes the utterances of a set's earlier
    subsets again for every further subset).
"""
from __future__ import annotations

import argparse
import os
import sys
from pathlib import Path

SET_NAMES = ("train", "dev", "test")
DEFAULT_LISTS = {"train": ["train-clean-100"], "dev": ["dev-clean", "dev-other"], "test": ["test-clean", "test-other"]}


def find_audios(directory, suffix=".flac"):
    """[(utterance id, path)] of every file below `directory` whose name ends in `suffix` (any letter case), by utterance id."""
    found = []
    for root, _, files in os.walk(directory):
        for name in files:
            if name.lower().endswith(suffix):
                found.append((os.path.splitext(name)[0], os.path.join(root, name)))
    return sorted(found)


def write_scp(root_dir, out_path, subset_list):
    """The utterances of the subsets of `subset_list` that exist under root_dir -> out_path; returns how many."""
    entries = []
    for subset in subset_list:
        if os.path.isdir(Path(root_dir) / subset):
            entries += find_audios(Path(root_dir) / subset)
    entries.sort()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        for uid, path in entries:
            fh.write(f"{uid} {path}\n")
    return len(entries)


def process_librispeech(raw_data_dir, output_dir, data_format="numpy", train_list=None, dev_list=None, test_list=None):
    """Writes <output_dir>/{train,dev,test}/wav.scp; returns the three paths."""
    print("Generating scp files...")
    lists = {"train": train_list, "dev": dev_list, "test": test_list}
    paths = []
    for name in SET_NAMES:
        scp = Path(output_dir) / name / "wav.scp"
        n = write_scp(raw_data_dir, scp, DEFAULT_LISTS[name] if lists[name] is None else lists[name])
        print(f"{name}: {n} utterances -> {scp}")
        paths.append(scp)
    print("Generated scp files")
    return tuple(paths)


def build_parser():
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("raw_data_dir", type=str, help="LibriSpeech raw data directory")
    p.add_argument("output_dir", type=str, help="Directory for data output")
    p.add_argument("--data-format", type=str, default="numpy", choices=["numpy", "kaldi"], help="Data format to use (the scp files are the same)")
    p.add_argument("--train_list", type=str, nargs="*", default=DEFAULT_LISTS["train"],
                   help="Training sets to include {train-clean-100, train-clean-360, train-other-500}")
    p.add_argument("--dev_list", type=str, nargs="*", default=DEFAULT_LISTS["dev"], help="Dev sets to include {dev-clean, dev-other}")
    p.add_argument("--test_list", type=str, nargs="*", default=DEFAULT_LISTS["test"], help="Test sets to include {test-clean, test-other}")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    print(args)
    process_librispeech(Path(args.raw_data_dir), Path(args.output_dir), args.data_format, args.train_list, args.dev_list, args.test_list)
    return 0


if __name__ == "__main__":
    sys.exit(main())
