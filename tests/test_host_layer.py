"""CPU-only: the host layer of the library (csrc/host.hpp, csrc/carver.hpp) and the one source list of every build.

 * every size query answers what tests/golden/workspace_sizes.json recorded (tools/record_workspace_sizes.py, run on the
   library as it was before the carves moved to one allocator): a carve edit that changes a size fails here, without a GPU;
 * the allocator alone, in a stand-alone program under AddressSanitizer and UBSan (tests/carver_check.cpp);
 * no script under tools/ carries a source list of its own, and a variant build compiles exactly build.SOURCES."""
import glob
import importlib.util
import json
import os
import re
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "workspace_sizes.json")


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _build_module():
    return _load("icpflow_build", os.path.join(REPO, "icp_flow_amd", "build.py"))


def test_every_size_query_answers_what_was_recorded():
    from icp_flow_amd import _lib
    recorded = json.load(open(GOLDEN))
    now = _load("record_workspace_sizes", os.path.join(REPO, "tools", "record_workspace_sizes.py")).measure(_lib)
    assert sorted(now) == sorted(recorded) and len(recorded) == 10
    compared = 0
    for query, rows in recorded.items():
        assert [r[:-1] for r in now[query]] == [r[:-1] for r in rows], query   # the same grid of shapes
        for was, row in zip(rows, now[query]):
            # (recorded without a device, where rocprim's scratch query fails for its longer sorts and the clustering queries
            # answer 0: those entries say nothing; icpflow_ground_workspace_bytes(0) is 0 by its contract and is compared)
            if was[-1] == 0 and query in ("icpflow_dbscan_workspace_bytes", "icpflow_hdbscan_mst_workspace_bytes"):
                continue
            assert row == was, (query, was, row)
            compared += 1
    assert compared >= 1500


def test_the_allocator_alone_under_sanitizers(tmp_path):
    recorded = dict((n, b) for n, b in json.load(open(GOLDEN))["icpflow_ground_workspace_bytes"])
    exe = str(tmp_path / "carver_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-g", "-O1", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(REPO, "tests", "carver_check.cpp"), "-o", exe])
    out = subprocess.run([exe, str(recorded[513])], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert out.stdout.strip() == f"ok {recorded[513]}" and out.stderr == ""


def test_no_tool_carries_a_source_list_of_its_own():
    """A hipcc argument list names several sources on one line; a comment or the one source a script rebuilds names one."""
    build = _build_module()
    as_path = re.compile(r"/(?:%s)(?![\w.])" % "|".join(re.escape(s) for s in build.SOURCES))   # .../api.hip, $C/icp.hip
    checked = 0
    for path in glob.glob(os.path.join(REPO, "tools", "**", "*"), recursive=True):
        if not os.path.isfile(path) or not path.endswith((".sh", ".py", ".hip", ".md")):
            continue
        checked += 1
        for k, line in enumerate(open(path, errors="replace"), 1):
            assert len(as_path.findall(line)) < 2, f"{os.path.relpath(path, REPO)}:{k} lists sources: build.py's SOURCES is the only list"
    assert checked >= 40


def test_a_variant_build_compiles_exactly_the_source_list(tmp_path):
    build = _build_module()
    out = str(tmp_path / "libvariant.so")
    plan = build.build(defines=["A=1", "B"], out=out, dry_run=True)
    assert not os.path.exists(out) and plan["out"] == out
    assert list(plan["compile"]) == build.SOURCES
    objs = []
    for src, argv in plan["compile"].items():
        stamp = [a for a in argv if a.startswith("-DICPFLOW_SOURCE_HASH=")]
        assert len(stamp) == (1 if src == "api.hip" else 0)
        assert argv[1:-4] == build.CFLAGS + ["-DA=1", "-DB"] + stamp, (src, argv)
        assert argv[-4:-1] == ["-c", os.path.join(build.CSRC, src), "-o"]
        objs.append(argv[-1])
        # a variant's objects are kept apart from the product's, whose cache it must not evict
        assert os.path.dirname(argv[-1]) != build.OBJ
    assert plan["link"][1:] == ["--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", out + ".tmp"]
    product = build.build(dry_run=True)
    assert product["out"] == build.OUT and all(os.path.dirname(a[-1]) == build.OBJ for a in product["compile"].values())
