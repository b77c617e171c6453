"""GPU: run_stream with all six judges on at once (residual, segments, line of sight, trust bytes, objects, tracks) against
what the same run gave at the commit before the judges moved out of run_stream into icp_flow_amd/pair_judges.py
(tests/golden/stream_judges/, recorded there by `record` below on an MI355X): the summary -- values and the order of the
keys at every level -- and the three files byte for byte, frame pair by frame pair and with three in flight.  The comparison
is exact because none of this depends on the order in which frame pairs complete (run_stream's docstring).  At that commit two
host sums still did, in their last bit -- the meter's weighted sums and the trust bytes' end-point errors were added as frame
pairs completed: two recordings and the run with three in flight agreed there, a later run with three in flight gave
`epe_kept` one unit in the last place away -- so both are now added in the order of the frame pairs, which is what the
fixtures hold (tests/test_frame_pairs.py delivers out of order without a GPU)."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_cases as tc                       # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stream_judges")
FILES = dict(residual_segments="segments.json", objects="objects.jsonl", tracks="tracks.jsonl")
KEPT, MISSING_IN_FRAME_0 = (0, 2, 3, tc.SCENE_WALL), 2
# wall-clock figures: every ms_* key, at every level, and the one rate that is not named so
TIMING = ("frame_pairs_per_s",)


def sample():
    """track_cases.scene() cut down to a few hundred points a frame: four of its five objects (the one that leaves its line
    among them), the two middle layers of their ten and the noise; object 2 is missing from frame 0, so its cluster in every
    source has nothing to fit to and the segments' list is not empty; `scene_flow` is the scene's truth.  -> the file's keys"""
    sc = tc.scene()
    arrays, obj = sc["arrays"], sc["object"]
    raw, frame = arrays["raw_points"], arrays["time_indice"]
    keep = (np.isin(obj, KEPT) & (np.abs(raw[:, 2] - tc.SCENE_CENTRES[0, 2]) < 0.1)) | (obj == -1)
    keep &= ~((obj == MISSING_IN_FRAME_0) & (frame == 0))
    flow = np.zeros((len(obj), 3))
    for k in KEPT:
        flow[obj == k] = -frame[obj == k, None] * tc.SCENE_STEPS[k]
    flow[(obj == tc.SCENE_BAD) & (frame == tc.SCENE_BAD_FRAME)] -= tc.SCENE_BAD_OFFSET
    flow[obj == -1, 1] = -frame[obj == -1]
    return dict(raw_points=raw[keep], time_indice=frame[keep], ego_motion=arrays["ego_motion"], scene_flow=flow[keep].astype(np.float32))


def untimed(value):
    """the summary without its wall-clock figures and the names of its files, the order of what stays kept"""
    if isinstance(value, dict):
        return {k: untimed(v) for k, v in value.items() if not (k.startswith("ms_") or k.endswith("_file") or k in TIMING)}
    return value


def run(in_flight):
    """run_stream over `sample.npz` of the CURRENT directory (the tracks' lines carry the path as given), every judge on
    -> (the summary's text, {file: its bytes})"""
    import torch
    from icp_flow_amd import frame_pairs
    a = frame_pairs.default_args(**tc.SCENE_CLUSTER)
    a.residual, a.residual_sight, a.residual_trust, a.sweep_seconds = 2.0, (0.0, 0.0, 0.0), True, tc.SCENE_SWEEP_SECONDS
    for attribute, name in FILES.items():
        setattr(a, attribute, f"{in_flight}_{name}")
    summary = frame_pairs.run_stream(a, ["sample.npz"], torch.device("cuda:0"), in_flight=in_flight)
    assert [summary[attribute + "_file"] for attribute in FILES] == [getattr(a, attribute) for attribute in FILES]
    files = {}
    for attribute, name in FILES.items():
        with open(getattr(a, attribute), "rb") as f:
            files[name] = f.read()
    return json.dumps(untimed(summary), indent=1) + "\n", files


def record(directory):
    """what the fixtures were written by (from a directory that holds sample()'s file): the run frame pair by frame pair, after
    checking that the run with three in flight gives the same"""
    text, files = run(1)
    assert (text, files) == run(3), "the parent disagrees with itself between in_flight = 1 and 3"
    os.makedirs(directory, exist_ok=True)
    with open(os.path.join(directory, "summary.json"), "w") as f:
        f.write(text)
    for name, data in files.items():
        with open(os.path.join(directory, name), "wb") as f:
            f.write(data)


@pytest.fixture(scope="module")
def directory(tmp_path_factory):
    root = tmp_path_factory.mktemp("stream_judges")
    np.savez(str(root / "sample.npz"), **sample())
    return root


@pytest.mark.parametrize("in_flight", (1, 3))
def test_every_judge_at_once_gives_what_the_parent_gave(directory, monkeypatch, in_flight):
    monkeypatch.chdir(directory)
    text, files = run(in_flight)
    with open(os.path.join(GOLDEN, "summary.json")) as f:
        want = f.read()
    summary = json.loads(text)
    assert summary["frame_pairs"] == 3 and summary["residual_segments"]["segments_listed"] > 0 and summary["tracks"]["tracks"] > 0
    assert list(summary) == list(json.loads(want)) and text == want
    for name, data in files.items():
        with open(os.path.join(GOLDEN, name), "rb") as f:
            assert data == f.read(), name
