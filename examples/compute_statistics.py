#!/usr/bin/env python
"""Mean and scale of a dumped feature on the MI355X engine -- the reference's utils/compute_statistics.py (:27-109) with
``parakeet_amd.normalizer.FeatureStats`` in the place of scikit-learn's ``StandardScaler.partial_fit``:

    python examples/compute_statistics.py --metadata dump/train/raw/metadata.jsonl --field-name speech

reads every ``<field-name>`` path of ``metadata.jsonl`` (one json record per line), feeds the arrays to the accumulator in
ragged batches of at most ``--batch-frames`` rows and writes the (2, D) float32 array [mean, scale] with ``np.save``; without
``--output`` to ``<parent of the metadata's directory>/<field-name>_stats.npy``, as the reference does.  Paths in the
metadata that are not absolute are taken relative to the metadata's directory (``--use-relative-path true`` in the
reference's preprocess.py writes such).  The result does not depend on ``--batch-frames``: the accumulator gives the same
bytes for any split at utterance boundaries.  NaN is not skipped (scikit-learn skips it).
"""
import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def read_metadata(path):
    with open(path, "rt", encoding="utf-8") as f:
        return [json.loads(line) for line in f if line.strip()]


def field_path(metadata_path, value, relative=False):
    p = Path(value)
    return p if p.is_absolute() and not relative else Path(metadata_path).parent / p


def compute(metadata_path, field_name, batch_frames=1 << 20, use_relative_path=False, stats_cls=None):
    """-> the fitted accumulator (``stats_cls``: a FeatureStats class; the default is the engine's)."""
    if stats_cls is None:
        from parakeet_amd.normalizer import FeatureStats as stats_cls
    acc, batch, frames = None, [], 0
    for item in read_metadata(metadata_path):
        x = np.load(field_path(metadata_path, item[field_name], use_relative_path), allow_pickle=False)
        if x.ndim == 1:
            x = x.reshape(-1, 1)
        if acc is None:
            acc = stats_cls(x.shape[1])
        if batch and frames + x.shape[0] > batch_frames:
            acc.partial_fit_batch(batch)
            batch, frames = [], 0
        batch.append(x)
        frames += x.shape[0]
    if acc is None:
        raise SystemExit(f"{metadata_path} has no records")
    if batch:
        acc.partial_fit_batch(batch)
    return acc


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Compute mean and scale of dumped raw features.")
    ap.add_argument("--metadata", type=str, required=True, help="jsonl file with ids and file paths")
    ap.add_argument("--field-name", type=str, required=True, help="name of the field to compute statistics for")
    ap.add_argument("--output", type=str, default=None,
                    help="where to save the statistics; by default <field-name>_stats.npy next to the metadata's directory")
    ap.add_argument("--use-relative-path", type=lambda s: s.lower() == "true", default=False,
                    help="the metadata's paths are relative to its directory")
    ap.add_argument("--batch-frames", type=int, default=1 << 20, help="most rows handed to the engine in one call")
    ap.add_argument("--verbose", type=int, default=1)
    return ap.parse_args(argv)


def main(argv=None, stats_cls=None):
    args = parse_args(argv)
    if args.batch_frames < 1:
        raise SystemExit("--batch-frames must be positive")
    out = Path(args.metadata).parent.with_name(args.field_name + "_stats.npy") if args.output is None else Path(args.output)
    out.parent.mkdir(parents=True, exist_ok=True)
    acc = compute(args.metadata, args.field_name, args.batch_frames, args.use_relative_path, stats_cls)
    with open(out, "wb") as f:                         # (np.save on a name would append .npy to one without it)
        np.save(f, acc.stats(), allow_pickle=False)
    if args.verbose > 0:
        print(f"{acc.n_samples_seen_} rows of {acc.dim} -> {out}")
    return out


if __name__ == "__main__":
    main()
