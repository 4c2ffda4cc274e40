#!/usr/bin/env python3
"""Time of the GPU MessageFormatSend (ambrycrc_send_messages_dev) over a region of m stored V3 PUTs with random
fields and blobs (made by the in-place serializer), against baselines timed in the same run, interleaved call by
call (HIP events around each call, median of --reps after a warm-up):

  send_blob / send_all / send_info   the three flags that matter for traffic: BLOB, ALL, BLOB_INFO
  transform      ambrycrc_transform_messages_dev on its general path (region mode off for that call): the same
                 read and write as BLOB / ALL, and more per message
  verify_jobs    ambrycrc_verify_messages_dev in job mode: what BLOB_INFO must stay below when blobs are large
  memcpy_*       one hipMemcpyAsync of the bytes each flag sends

The first send of each flag is checked: every message sent with check 0, spans packed back to back, and the
output equal to the stored bytes at the reported offsets. Prints one JSON line per case."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CASES = {"4k": (262144, 4096), "64k": (65536, 65536)}


def run(m, blob_bytes, reps, only=None):
    import numpy as np
    import torch

    from ambry_amd import device as D
    from ambry_amd import messages as M
    from bench_put import _props_tensor

    key_len, props_len, um_len = 24, 94, 1000
    L, fo = M.layout(M.PutMessage(key=bytes(key_len), props=bytes(props_len), usermeta=bytes(um_len),
                                  blob=bytes(blob_bytes)))
    descs = np.zeros(m, dtype=M.PUT_DESC_DTYPE)
    idx = np.arange(m, dtype=np.uint64)
    descs["out_off"] = idx * L
    descs["blob_len"] = blob_bytes
    descs["key_len"], descs["props_len"], descs["usermeta_len"] = key_len, props_len, um_len
    descs["enckey_len"] = -1
    descs["header_version"] = 3
    region = torch.empty(m * L, dtype=torch.uint8, device="cuda")
    D.fill_random(region[: (m * L) // 16 * 16], 3, 0)
    p0 = fo["props"]
    region.view(m, L)[:, p0:p0 + props_len] = _props_tensor(torch)
    M.serialize_dev(torch.from_numpy(descs.view(np.uint8).copy()).cuda(), region)  # in place: random fields
    offs = torch.from_numpy((idx * L).astype(np.int64)).cuda()
    out = torch.empty(M.out_bound(region.numel(), m), dtype=torch.uint8, device="cuda")
    ws = torch.empty(M.send_workspace_bytes(m), dtype=torch.uint8, device="cuda")

    # the spans of one message, relative to it: (offset, length) per flag
    props_rel, um_rel, blob_rel = p0 - 2, fo["usermeta"] - 6, fo["blob"] - 13
    span = {"send_blob": (M.SEND_BLOB, blob_rel, L - blob_rel), "send_all": (M.SEND_ALL, 0, L),
            "send_info": (M.SEND_BLOB_INFO, props_rel, blob_rel - props_rel)}
    for name, (flag, rel, n) in span.items():  # a check of the whole pipeline once per flag
        _, info, st = M.send_messages_dev(region, offs, flag, out=out, workspace=ws)
        torch.cuda.synchronize()
        assert int(st.abs().sum().item()) == 0, name
        f = info.cpu().numpy().view(M.SEND_INFO_DTYPE)
        assert not f["check"].any() and (f["send_len"] == n).all() and (f["rel_off"] == rel).all(), name
        assert (f["out_off"] == idx * np.uint64(n)).all(), name
        assert bool(torch.equal(out[: m * n].view(m, n), region.view(m, L)[:, rel:rel + n])), name

    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    mode = D.get_region_mode(0)

    def region_off(fn):
        def call():
            D.set_region_mode(0, 0)  # job mode / the transform's general path
            try:
                fn()
            finally:
                D.set_region_mode(0, mode)
        return call

    def send(flag):
        return lambda: M.send_messages_dev(region, offs, flag, out=out, workspace=ws)

    def memcpy(nbytes):
        return lambda: hip.hipMemcpyAsync(out.data_ptr(), region.data_ptr(), nbytes, 3, stream)

    calls = {
        "send_blob": send(M.SEND_BLOB), "send_all": send(M.SEND_ALL), "send_info": send(M.SEND_BLOB_INFO),
        "transform": region_off(lambda: M.transform_dev(region, offs, out=out)),
        "verify_jobs": region_off(lambda: D.verify_messages(region, offs, want_end=False)),
        "memcpy_blob": memcpy(m * span["send_blob"][2]), "memcpy_all": memcpy(m * L),
        "memcpy_info": memcpy(m * span["send_info"][2]),
    }
    if only:  # a profiler run of some calls alone
        calls = {k: v for k, v in calls.items() if k in only}

    def once(name):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        calls[name]()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    t_pre = time.perf_counter()
    while time.perf_counter() - t_pre < 0.5:
        for name in calls:
            once(name)
    if "transform" in calls:
        once("transform")
        assert D.last_transform_path(0) == 0
    if "verify_jobs" in calls:
        once("verify_jobs")
        assert D.last_message_mode(0) == 0
    times = {name: [] for name in calls}
    for _ in range(reps):  # interleaved: every call sees the same machine state over the run
        for name in calls:
            times[name].append(once(name))
    ms = {name: sorted(t)[len(t) // 2] for name, t in times.items()}
    lo = {name: min(t) for name, t in times.items()}
    hi = {name: max(t) for name, t in times.items()}
    res = {"case": f"send {m} x PUT({blob_bytes} B blob)", "messages": m, "region_bytes": m * L, "reps": reps,
           "sent_bytes": {k: m * v[2] for k, v in span.items()},
           "ms_median": {k: round(x, 4) for k, x in ms.items()}, "ms_min": {k: round(x, 4) for k, x in lo.items()},
           "ms_max": {k: round(x, 4) for k, x in hi.items()}}
    if not only:
        res.update({
            "send_blob_over_transform": round(ms["send_blob"] / ms["transform"], 3),
            "send_all_over_transform": round(ms["send_all"] / ms["transform"], 3),
            "transform_spread": round((hi["transform"] - lo["transform"]) / ms["transform"], 3),
            "send_info_over_verify_jobs": round(ms["send_info"] / ms["verify_jobs"], 3),
            "send_blob_over_memcpy": round(ms["send_blob"] / ms["memcpy_blob"], 3),
            "send_all_over_memcpy": round(ms["send_all"] / ms["memcpy_all"], 3),
            "send_info_over_memcpy": round(ms["send_info"] / ms["memcpy_info"], 3),
            "send_blob_GBps_sent": round(m * span["send_blob"][2] / (ms["send_blob"] / 1e3) / 1e9, 1),
            "parity": "every message sent with check 0, spans packed, output equal to the stored bytes"})
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default="4k,64k", help="comma list of %s" % ",".join(CASES))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--only", default=None, help="comma list of calls to time alone: a profiler run; no ratios")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    import torch

    from ambry_amd import device as D

    if not torch.cuda.is_available():
        raise SystemExit("bench_send: needs a GPU (no CPU fallback for a timing)")
    torch.cuda.set_device(0)
    D.init(0)
    for name in args.cases.split(","):
        m, blob = CASES[name]
        line = json.dumps(run(m, blob, args.reps, args.only.split(",") if args.only else None))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
