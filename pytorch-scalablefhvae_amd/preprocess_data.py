"""preprocess_data.py -- from a raw LibriSpeech or TIMIT directory to features, in one command (the reference's
preprocess_data.py): the wav.scp files of the three sets (preprocess_librispeech.py / preprocess_timit.py), then the features
of each set (prepare_numpy_data.py or prepare_kaldi_data.py), all audio decoding and feature arithmetic on the GPU.

    python pytorch-scalablefhvae_amd/preprocess_data.py {librispeech,timit} RAW_DATA_DIR [--data-format {numpy,kaldi}]
        [--feat-type {fbank,spec}] [--sample-rate RATE] [--win-size 0.025] [--hop-size 0.010] [--mels 80]
        [--fbank-conf ./misc/fbank.conf] [--dev-spk LIST --test-spk LIST] [--verify-md5]

The output directory is <dataset>_np_<feat type> or <dataset>_kd_fbank under the working directory, as in the reference.
preprocess_data(args) returns the reference's paths_dict: per set the paths under "wav_pth", "feat_pth", "len_pth" (numpy) or
"wav_pth", "feat_ark", "feat_pth", "len_pth" (kaldi), in the order the prepare functions return them.

Differences from the reference:
  * the three sets run one after the other on the GPU, not in a pool of three processes.
  * there is no --kaldi-root: no Kaldi binary is run.
  * --sample-rate maps to the prepare tools' --resample --sr: with it files at other rates are converted on the GPU, without
    it every file of a set must have one rate.  For the kaldi format the target is the configuration's sample-frequency, and a
    --sample-rate that differs from it is an error.
  * timit needs --dev-spk and --test-spk (see preprocess_timit.py); librispeech audio stays FLAC, timit audio stays SPHERE.
"""
from __future__ import annotations

import argparse
import os
import sys
import time
from pathlib import Path

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

DATA_SETS = ("train", "dev", "test")


def output_dir_name(dataset, data_format, feat_type):
    """<dataset>_np_<feat type>, or <dataset>_kd_fbank (the Kaldi format has filterbank features only)."""
    return Path("%s_%s_%s" % (dataset, "np" if data_format.lower() == "numpy" else "kd", feat_type if data_format != "kaldi" else "fbank"))


def preprocess_data(args):
    from prepare_kaldi_data import prepare_kaldi
    from prepare_numpy_data import prepare_numpy
    from preprocess_librispeech import process_librispeech
    from preprocess_timit import process_timit

    dataset_directory = output_dir_name(args.dataset, args.data_format, args.feat_type)
    verify = getattr(args, "verify_md5", False)
    if args.dataset == "timit":
        if not getattr(args, "dev_spk", None) or not getattr(args, "test_spk", None):
            raise ValueError("timit needs --dev-spk and --test-spk, the lists of dev and test speakers")
        process_timit(Path(args.raw_data_dir).resolve(), dataset_directory, args.dev_spk, args.test_spk)
    else:
        process_librispeech(Path(args.raw_data_dir).resolve(), dataset_directory, args.data_format)
    start = time.time()
    results = []
    for set_name in DATA_SETS:
        if args.data_format == "numpy":
            results.append(prepare_numpy(args.dataset, set_name, dataset_directory, None, args.feat_type, args.sample_rate, args.win_size,
                                         args.hop_size, args.mels, resample=args.sample_rate is not None, verify_md5=verify))
        else:
            if args.sample_rate is not None:
                import features

                conf_sr = int(features.kaldi_fbank_options(args.fbank_conf)["sample-frequency"])
                if conf_sr != args.sample_rate:
                    raise ValueError("--sample-rate %d differs from sample-frequency %d of %s" % (args.sample_rate, conf_sr, args.fbank_conf))
            results.append(prepare_kaldi(dataset_directory, set_name, args.fbank_conf, resample=args.sample_rate is not None, verify_md5=verify))
    print(f"Processed {sum(r[0] for r in results)} files in {time.time() - start:.2f} seconds.")
    keys = ("wav_pth", "feat_pth", "len_pth") if args.data_format == "numpy" else ("wav_pth", "feat_ark", "feat_pth", "len_pth")
    return {name: dict(zip(keys, r[1])) for name, r in zip(DATA_SETS, results)}


def build_parser():
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("dataset", type=str, choices=["librispeech", "timit"], help="Dataset to preprocess")
    p.add_argument("raw_data_dir", type=str, help="Location for raw data")
    p.add_argument("--data-format", type=str, default="numpy", choices=["numpy", "kaldi"], help="Data format to use for precomputed features")
    p.add_argument("--fbank-conf", type=str, default="./misc/fbank.conf", help="Kaldi fbank configuration")
    p.add_argument("--feat-type", type=str, default="fbank", choices=["fbank", "spec"], help="Feature type to compute (only affects numpy data)")
    p.add_argument("--hop-size", type=float, default=0.010, help="Frame spacing in seconds")
    p.add_argument("--mels", type=int, default=80, help="Number of filter banks if choosing fbank")
    p.add_argument("--sample-rate", type=int, default=None, help="Resample raw audio to specified value if not None")
    p.add_argument("--win-size", type=float, default=0.025, help="Window size in seconds")
    p.add_argument("--dev-spk", type=str, default=None, help="timit: path to list of dev set speakers")
    p.add_argument("--test-spk", type=str, default=None, help="timit: path to list of test set speakers")
    p.add_argument("--verify-md5", action="store_true", help="Check every FLAC file's decoded audio against the MD5 it carries")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    try:
        preprocess_data(args)
    except ValueError as e:
        print("preprocess_data: %s" % e, file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
