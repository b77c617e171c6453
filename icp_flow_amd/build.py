"""Build libicpflow_hip.so in-tree with hipcc for gfx950 (no torch, no cmake).

    python icp_flow_amd/build.py [--force] [--save-temps]
    python icp_flow_amd/build.py --define NAME[=VALUE] ... --out PATH [--dry-run]     an instrumented variant

hipcc cross-compiles without a GPU; the .so travels with the tree to the GPU box.  Every source is
compiled to its own object (in parallel, cached by content hash under csrc/_obj/) and linked once.
Flags that matter for parity:
  -ffp-contract=off                         every FMA in the kernels is an explicit fmaf()
  -fhip-fp32-correctly-rounded-divide-sqrt  IEEE division in the vote's bin index and
                                            correctly rounded sqrt of the NN distances
The library carries the hash of the sources it was built from (icpflow_build_info()); a library whose
hash differs from the tree's is stale and rebuilt, whatever the file times say.

SOURCES, HEADERS and CFLAGS below are the only copy of what the library is built from.  A variant (tools/dbg: the same
sources with extra -D defines, linked to a path of its own) is built by build(defines=..., out=...); its objects are cached
under csrc/_obj/variant/, so it neither replaces the product library nor evicts the product's objects.
"""
import argparse
import concurrent.futures
import hashlib
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(CSRC, "_obj")
OUT = os.path.join(HERE, "libicpflow_hip.so")
SOURCES = ["api.hip", "hist.hip", "nn.hip", "icp.hip", "icp_prep.hip", "icp_plan.hip", "icp_epilogue.hip", "device.hip", "icp_fp32.hip", "pose.hip", "sort.hip", "cluster.hip", "hdbscan.hip", "clusterpcd.hip", "table.hip", "assoc.hip", "frame.hip", "ego.hip", "seqeval.hip", "classeval.hip", "bucketeval.hip", "segeval.hip", "ground.hip", "nnresid.hip", "segresid.hip", "sight.hip", "trust.hip", "boxes.hip", "overlap.hip", "tracks.hip", "carry.hip", "repair.hip",
           "hdbscan_tree.cpp"]
HEADERS = ["common.hpp", "scan.hpp", "kernels.hpp", "kabsch.hpp", "posefuse.hpp", "scorepick.hpp", "votekey.hpp", "cluster_util.hpp", "sortdir.hpp", "sortclouds.hpp", "occgrid.hpp", "host.hpp", "carver.hpp", "rowerr.hpp", "clusterpcd_host.hpp", "gridhash.hpp", "nnresid.hpp", "sight.hpp", "labelkey.hpp", "trust.hpp", "boxes.hpp", "overlap.hpp", "rejecttest.hpp", "icp_instr.hip",
           os.path.join("..", "..", "include", "icpflow_hip.h")]
CFLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
          "-fhip-fp32-correctly-rounded-divide-sqrt", "-Wall", "-Wno-unused-function"]


def hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    return "hipcc"


def _digest(paths, extra=()):
    h = hashlib.sha256()
    for p in paths:
        h.update(os.path.basename(p).encode())
        with open(p, "rb") as f:
            h.update(f.read())
    for e in extra:
        h.update(str(e).encode())
    return h.hexdigest()


def source_hash():
    """Hash of everything the library is built from (sources, headers, flags)."""
    return _digest([os.path.join(CSRC, f) for f in SOURCES + HEADERS], CFLAGS)[:16]


_MARK = b"ICPFLOW_SOURCE_HASH="


def built_hash(path=OUT):
    """The source hash baked into an existing library, or None.  Read from the file's bytes: loading the library
    here would pull the system HIP runtime into the process before torch brings its own (two runtimes in one
    process do not share devices)."""
    try:
        with open(path, "rb") as f:
            blob = f.read()
    except OSError:
        return None
    k = blob.find(_MARK)
    if k < 0:
        return None
    tag = blob[k + len(_MARK): k + len(_MARK) + 16]
    return tag.decode() if len(tag) == 16 and all(c in b"0123456789abcdef" for c in tag) else None


def stale():
    return built_hash() != source_hash()


def _object(src, extra, objdir):
    hdr = _digest([os.path.join(CSRC, f) for f in HEADERS], CFLAGS + list(extra))
    tag = _digest([os.path.join(CSRC, src)], [hdr])[:16]
    return os.path.join(objdir, f"{os.path.splitext(src)[0]}.{tag}.o")


def _compile(src, obj, argv):
    if not os.path.exists(obj) or "-save-temps=obj" in argv:
        os.makedirs(os.path.dirname(obj), exist_ok=True)
        for old in os.listdir(os.path.dirname(obj)):   # (the older objects of this source, in this directory only)
            if old.startswith(os.path.splitext(src)[0] + ".") and old.endswith(".o"):
                os.remove(os.path.join(os.path.dirname(obj), old))
        subprocess.check_call(argv, cwd=CSRC)
    return obj


def plan(defines=(), out=None, extra=()):
    """The commands of one build, nothing run: {"compile": {source: argv}, "link": argv, "out": path}.  With an `out` of
    its own it is a variant: every source of SOURCES with CFLAGS and -D<d> for each d of `defines` (["NAME", "NAME=VALUE",
    ...]), objects under csrc/_obj/variant/."""
    out = os.path.abspath(out) if out else OUT
    variant = out != OUT
    if defines and not variant:
        raise ValueError("a build with defines is a variant: give it an `out` of its own (the product library is built as shipped)")
    objdir = os.path.join(OBJ, "variant") if variant else OBJ
    extra = list(extra) + ["-D" + d for d in defines]
    stamp = source_hash()
    compile_, objs = {}, []
    for src in SOURCES:
        # only api.hip sees the hash (the other objects stay cached when an unrelated file changes)
        e = extra + ([f'-DICPFLOW_SOURCE_HASH="{stamp}"'] if src == "api.hip" else [])
        objs.append(_object(src, e, objdir))
        compile_[src] = [hipcc()] + CFLAGS + e + ["-c", os.path.join(CSRC, src), "-o", objs[-1]]
    return {"compile": compile_, "link": [hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", out + ".tmp"], "out": out}


def build(force=False, extra=(), defines=(), out=None, dry_run=False):
    """Build the product library (only when it is stale, or with force) or, with defines / out, a variant (always linked
    anew).  dry_run: -> plan(), nothing compiled."""
    p = plan(defines, out, extra)
    if dry_run:
        return p
    if p["out"] == OUT and not force and not stale():
        return OUT
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(len(SOURCES), os.cpu_count() or 1)) as ex:
        jobs = [ex.submit(_compile, src, argv[-1], argv) for src, argv in p["compile"].items()]
        for j in jobs:
            j.result()
    subprocess.check_call(p["link"], cwd=CSRC)
    os.replace(p["out"] + ".tmp", p["out"])
    return p["out"]


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--force", action="store_true")
    ap.add_argument("--save-temps", action="store_true")
    ap.add_argument("--define", action="append", default=[], metavar="NAME[=VALUE]", help="build a variant with -DNAME[=VALUE] (repeatable)")
    ap.add_argument("--out", metavar="PATH", help="where the variant is linked to")
    ap.add_argument("--dry-run", action="store_true", help="print the commands, run nothing")
    a = ap.parse_args()
    extra = ["-save-temps=obj"] if a.save_temps else []
    res = build(force=a.force or bool(extra), extra=extra, defines=a.define, out=a.out, dry_run=a.dry_run)
    if a.dry_run:
        for argv in list(res["compile"].values()) + [res["link"]]:
            print(" ".join(argv))
    else:
        print(res, source_hash())
