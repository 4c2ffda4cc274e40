#!/usr/bin/env python3
"""Time of the GPU hard delete (ambrycrc_hard_delete_messages_dev) over a region of m stored V3 PUTs with
random fields and blobs (made by the in-place serializer), against baselines timed in the same run,
interleaved call by call (HIP events around each call, median of --reps after a warm-up):

  fill call   the second phase, with the first phase's recovery info: header checks and a store stream.
              Baseline: one hipMemsetAsync of a contiguous buffer of as many bytes as the call zeroes.
  full call   no recovery info: the user-metadata and blob records verified, then rewritten.
              Baseline: ambrycrc_verify_messages_dev on the same region plus that memset.
  plan call   plan_only (checks and recovery info, no write), for the breakdown.

The region is restored from a copy before every call that reads the records (outside the timed span). The
first full call is checked: every message deleted, every message verifies clean afterwards, the bodies are
zero. Prints one JSON line per case."""
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

CASES = {"4k": (262144, 4096), "64k": (65536, 65536), "4m": (1024, 4 << 20)}


def run(m, blob_bytes, reps):
    import numpy as np
    import torch

    from ambry_amd import device as D
    from ambry_amd.messages import PUT_DESC_DTYPE, PutMessage, layout, serialize_dev
    from bench_put import _props_tensor

    key_len, props_len, um_len = 24, 94, 1000
    L, fo = layout(PutMessage(key=bytes(key_len), props=bytes(props_len), usermeta=bytes(um_len),
                              blob=bytes(blob_bytes)))
    descs = np.zeros(m, dtype=PUT_DESC_DTYPE)
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
    serialize_dev(torch.from_numpy(descs.view(np.uint8).copy()).cuda(), region)  # in place: random fields
    offs = torch.from_numpy((idx * L).astype(np.int64)).cuda()
    saved = region.clone()
    zeroed = m * (um_len + blob_bytes)
    flat = torch.empty(zeroed, dtype=torch.uint8, device="cuda")
    D.fill_random(flat[: zeroed // 16 * 16], 4, 0)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]

    # the first phase, and a check of the whole pipeline once
    st, info = D.hard_delete_messages(region, offs, plan_only=True)
    torch.cuda.synchronize()
    assert int(st.abs().sum().item()) == 0 and bool(torch.equal(region, saved))
    st, info2 = D.hard_delete_messages(region, offs)
    vst, _ = D.verify_messages(region, offs, want_end=False)
    torch.cuda.synchronize()
    assert int(st.abs().sum().item()) == 0 and int(vst.abs().sum().item()) == 0 and bool(torch.equal(info, info2))
    um0, b0 = fo["usermeta"], fo["blob"]
    v = region.view(m, L)
    assert int(v[:, um0:um0 + um_len].max().item()) == 0 and int(v[:, b0:b0 + blob_bytes].max().item()) == 0
    keep = torch.ones(L, dtype=torch.bool, device="cuda")  # every byte outside the two records is as before
    keep[um0 - 6:] = False
    assert bool(torch.equal(v[:, keep], saved.view(m, L)[:, keep]))

    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    calls = {
        "full": (True, lambda: D.hard_delete_messages(region, offs)),
        "fill": (False, lambda: D.hard_delete_messages(region, offs, recovery=info)),
        "plan": (True, lambda: D.hard_delete_messages(region, offs, plan_only=True)),
        "verify": (True, lambda: D.verify_messages(region, offs, want_end=False)),
        "memset": (False, lambda: hip.hipMemsetAsync(flat.data_ptr(), 0, zeroed, stream)),
    }

    def once(name):
        restore, fn = calls[name]
        if restore:
            region.copy_(saved)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    t_pre = time.perf_counter()
    while time.perf_counter() - t_pre < 0.5:
        for name in calls:
            once(name)
    times = {name: [] for name in calls}
    for _ in range(reps):  # interleaved: every call sees the same machine state over the run
        for name in calls:
            times[name].append(once(name))
    ms = {name: sorted(t)[len(t) // 2] for name, t in times.items()}
    lo = {name: min(t) for name, t in times.items()}
    return {"case": f"hard delete {m} x PUT({blob_bytes} B blob)", "messages": m, "region_bytes": m * L,
            "zeroed_bytes": zeroed, "reps": reps,
            "ms_median": {k: round(x, 4) for k, x in ms.items()}, "ms_min": {k: round(x, 4) for k, x in lo.items()},
            "memset_GBps": round(zeroed / (ms["memset"] / 1e3) / 1e9, 1),
            "fill_call_GBps_zeroed": round(zeroed / (ms["fill"] / 1e3) / 1e9, 1),
            "fill_call_over_memset": round(ms["fill"] / ms["memset"], 3),
            "full_call_over_verify_plus_memset": round(ms["full"] / (ms["verify"] + ms["memset"]), 3),
            "verify_mode": D.last_message_mode(0),
            "parity": "every message deleted and clean under ambrycrc_verify_messages_dev, bodies zero, "
                      "bytes outside the two records unchanged"}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default="4k,64k,4m", help="comma list of %s" % ",".join(CASES))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    import torch

    from ambry_amd import device as D

    if not torch.cuda.is_available():
        raise SystemExit("bench_hard_delete: needs a GPU (no CPU fallback for a timing)")
    torch.cuda.set_device(0)
    D.init(0)
    for name in args.cases.split(","):
        m, blob = CASES[name]
        line = json.dumps(run(m, blob, args.reps))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
