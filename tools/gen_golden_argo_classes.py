#!/usr/bin/env python3
"""Generate tests/golden/g16_argo_classes.json: the lists of names and settings the REFERENCE's Argoverse 2 loader carries for
reporting per class and per speed (dataset_argo.py:145-217), read from its module the way tools/gen_golden_argo.py reads it.
Runs only where the reference is; the fixture holds names and numbers, no reference source text.

Recorded: the category names by the position the reference compares a file's classes with (its id table sorted by id), the
four meta categories as lists of names, the speed and end-point-error splits (inf as the string "inf"), and the background
indexes its Dataset_argo computes.  tests/test_classes.py holds icp_flow_amd.utils_eval's constants against them.

Usage:  python tools/gen_golden_argo_classes.py
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, REPO)
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REPO, "tools", "standins"))

import matplotlib  # noqa: E402

matplotlib.use("Agg")

import dataset_argo  # noqa: E402  (reference)

OUT = os.path.join(REPO, "tests", "golden", "g16_argo_classes.json")


def number(x):
    return "inf" if x == float("inf") else float(x)


def main():
    by_position = sorted(dataset_argo.CATEGORY_NAME_TO_IDX.items(), key=lambda kv: kv[1])
    assert [p for _, p in by_position] == list(range(len(by_position)))
    out = dict(generator="tools/gen_golden_argo_classes.py",
               names_by_position=[name for name, _ in by_position],
               first_id=int(min(dataset_argo.CATEGORY_ID_TO_NAME)),
               meta={k: list(v) for k, v in dataset_argo.METACATAGORIES.items()},
               speed_splits_m_per_s=[number(x) for x in dataset_argo.SPEED_BUCKET_SPLITS_METERS_PER_SECOND],
               error_splits_m=[number(x) for x in dataset_argo.ENDPOINT_ERROR_SPLITS_METERS],
               background_idxes=[int(dataset_argo.CATEGORY_NAME_TO_IDX[c]) for c in dataset_argo.METACATAGORIES["BACKGROUND"]])
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {OUT}  ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
