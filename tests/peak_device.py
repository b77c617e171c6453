"""What the GPU tests of the peak search share, in the style of tests/match_eval_device.py: the raw call of icpflow_hist_peaks (float
bins) or icpflow_selftest_peaks_u32 (the pipeline's instantiation: uint32 counters, the fused candidate decode) on buffers the
test owns -- a workspace of EXACTLY the documented size, filled with 0xFF, between two guards; votes, indices and candidates between
guards in allocations of their own, poisoned beforehand, every word written -- and the comparison with tests/peak_restatement.py.
Everything is array_equal: the operation is integer maxima and comparisons.  Not a test module."""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import peak_cases as pc                  # noqa: E402
import peak_restatement as pr            # noqa: E402
import residual_device as rd             # noqa: E402

GUARD, DEV = rd.GUARD, rd.DEV
WS_POISON, OUT_POISON = 0xFF, 0xA5
F32_EXACT = 1 << 24                      # float bins hold every integer below this exactly


def workspace_bytes(B, L):
    """include/icpflow_hip.h: two scratch volumes of B L uint32 words, each rounded up to a multiple of 256 bytes."""
    return 2 * (-(-(B * L * 4) // 256) * 256)


def run(vol, k, ks, entry="f32", stream=None, decode=True):
    """One call on `vol` (int64 [B, Lx, Ly, Lz]) -> dict(votes float32 [B, k], idx int64 [B, k], cand float32 [B, k + 1, 3] or None).
    Status 0, every guard intact, every output word written."""
    from icp_flow_amd import _lib
    L_, ptr = _lib._L, _lib.ptr
    B, Lx, Ly, Lz = (int(n) for n in vol.shape)
    if entry == "f32":
        assert int(vol.max()) < F32_EXACT
        bins = torch.from_numpy(vol.astype(np.float32)).to(DEV)
    else:
        bins = torch.from_numpy(vol.astype(np.uint32).view(np.int32)).to(DEV)
    need = workspace_bytes(B, Lx * Ly * Lz)
    ws = rd._guarded(need, WS_POISON)
    with_cand = entry == "u32" and decode
    sizes = dict(votes=B * k * 4, idx=B * k * 8)
    if with_cand:
        sizes["cand"] = B * (k + 1) * 3 * 4
    bufs = {n: rd._guarded(v, OUT_POISON) for n, v in sizes.items()}
    at = lambda b: ctypes.c_void_p(b.data_ptr() + GUARD)   # noqa: E731
    e = [torch.from_numpy(x).to(DEV) for x in pc.edges((Lx, Ly, Lz))]
    torch.cuda.synchronize()                                # (the uploads and the poison ran on the default stream)
    with torch.cuda.stream(stream):
        if entry == "f32":
            rc = L_.icpflow_hist_peaks(ptr(bins), B, Lx, Ly, Lz, k, ks, at(bufs["votes"]), at(bufs["idx"]), at(ws), need, _lib.stream(DEV))
        else:
            rc = L_.icpflow_selftest_peaks_u32(ptr(bins), B, Lx, Ly, Lz, k, ks, ptr(e[0]), ptr(e[1]), ptr(e[2]), pc.SHIFT, at(bufs["votes"]),
                                               at(bufs["idx"]), at(bufs["cand"]) if with_cand else None, at(ws), need, _lib.stream(DEV))
    msg = L_.icpflow_last_error().decode() if rc else ""
    torch.cuda.synchronize()
    assert rc == 0, (rc, msg)
    assert rd._guards_intact(ws, need), "guard of the workspace changed"
    out = dict(cand=None)
    for n, dt, shape in (("votes", torch.int32, (B, k)), ("idx", torch.int64, (B, k)), ("cand", torch.int32, (B, k + 1, 3))):
        if n not in bufs:
            continue
        assert rd._guards_intact(bufs[n], sizes[n]), f"guard of {n} changed"
        words = bufs[n][GUARD: GUARD + sizes[n]].clone().view(dt).cpu().numpy().reshape(shape)
        # (0xA5A5A5A5 is the float32 -2.87e-16 and a negative index: no result of any case)
        poison = np.uint32(0xA5A5A5A5) if dt == torch.int32 else np.uint64(0xA5A5A5A5A5A5A5A5)
        assert not (words.view(poison.dtype) == poison).any(), f"{n}: words left unwritten"
        out[n] = words if n == "idx" else words.view(np.float32)
    return out


def same_bits(a, b):
    return all((a[n] is None and b[n] is None) or np.array_equal(np.ascontiguousarray(a[n]).view(np.uint8), np.ascontiguousarray(b[n]).view(np.uint8))
               for n in ("votes", "idx", "cand"))


_SECOND = []


def second_stream():
    if not _SECOND:
        _SECOND.append(torch.cuda.Stream(device=DEV))
    return _SECOND[0]


def check(case, ks=None, k=None):
    """Both entries on a case against the restatement: the float one where the votes fit a float, the uint32 one with its decode;
    each once more on the same stream and on a second one, bit for bit the same.  -> the restatement's (votes, idx)"""
    vol, ks, k = case["vol"], ks or case["ks"], k or case["k"]
    wv, wi = pr.peaks(vol, k, ks)
    wc = pr.candidates(wi, vol.shape[1:], pc.edges(vol.shape[1:]), pc.SHIFT)
    label = (case["name"], ks, k)
    for entry in ("f32", "u32"):
        if entry == "f32" and int(vol.max()) >= F32_EXACT:
            continue
        got = run(vol, k, ks, entry)
        bad = np.flatnonzero((got["idx"] != wi).any(axis=1) | (got["votes"] != wv).any(axis=1))
        first = int(bad[0]) if len(bad) else 0
        assert np.array_equal(got["idx"], wi), (label, entry, "idx", len(bad), "volumes differ; first:", first, got["idx"][first], wi[first])
        assert np.array_equal(got["votes"], wv), (label, entry, "votes", len(bad), "volumes differ; first:", first, got["votes"][first], wv[first])
        if got["cand"] is not None:
            assert np.array_equal(got["cand"].view(np.uint32), wc.view(np.uint32)), (label, "candidates", got["cand"][0], wc[0])
            assert not got["cand"][:, -1].view(np.uint32).any(), (label, "the zero translation comes last")
        assert same_bits(got, run(vol, k, ks, entry)), (label, entry, "a rerun differs")
        assert same_bits(got, run(vol, k, ks, entry, stream=second_stream())), (label, entry, "a run on a second stream differs")
    return wv, wi
