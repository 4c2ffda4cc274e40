#!/usr/bin/env python3
"""Time of the GPU re-key (ambrycrc_rekey_messages_dev) over a region of m stored V3 PUTs with random fields
and blobs (made by the in-place serializer), against baselines timed in the same run, interleaved call by call
(HIP events around each call, median of --reps after a warm-up):

  rekey_same   (a) new keys of the stored keys' length
  rekey_long   (b) new keys 16 B longer: every record lands at another alignment
  transform    (c) ambrycrc_transform_messages_dev on its general path (region mode off for that call),
               which moves the same bytes
  memcpy       (d) one hipMemcpyAsync of the region

The first re-key of each kind is checked: every message re-keyed, every output clean under
ambrycrc_verify_messages_dev, the new keys in place. After the timed runs one re-key runs with the library's
sweep timing on (ambrycrc_timing_collect_each): its two CRC sweeps (the verify's and the replacement contents',
empty here) against the whole call. Prints one JSON line per case."""
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

    grow = 16
    aux = torch.empty(m * (key_len + grow), dtype=torch.uint8, device="cuda")
    D.fill_random(aux[: aux.numel() // 16 * 16], 5, 0)
    rk = {}
    for name, kl in (("rekey_same", key_len), ("rekey_long", key_len + grow)):
        d = np.zeros(m, dtype=M.REKEY_DESC_DTYPE)
        d["key_src"], d["key_len"] = idx * kl, kl
        d["content_src"], d["props_blob_size"] = M.REKEY_KEEP, -1
        d["account_id"], d["container_id"] = 1234, 56
        rk[name] = (kl, torch.from_numpy(d.view(np.uint8).copy()).cuda())
    out = torch.empty(M.rekey_out_bound(region.numel(), m, aux.numel()), dtype=torch.uint8, device="cuda")
    ws = torch.empty(M.rekey_workspace_bytes(m), dtype=torch.uint8, device="cuda")

    for name, (kl, dd) in rk.items():  # a check of the whole pipeline once per kind
        _, ooff, olen, st = M.rekey_dev(region, offs, dd, aux, out=out, workspace=ws)
        torch.cuda.synchronize()
        assert int(st.abs().sum().item()) == 0, name
        Lo = L + kl - key_len
        assert bool((olen == Lo).all()) and bool(torch.equal(ooff, torch.arange(m, device="cuda") * Lo))
        vst, _ = D.verify_messages(out[: m * Lo], ooff, want_end=False)
        torch.cuda.synchronize()
        assert int(vst.abs().sum().item()) == 0, name
        assert bool(torch.equal(out[: m * Lo].view(m, Lo)[:, 40:40 + kl], aux[: m * kl].view(m, kl))), name

    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    mode = D.get_region_mode(0)

    def transform_general():
        D.set_region_mode(0, 0)  # the general path: verify jobs with copy-through, layout, seal
        try:
            M.transform_dev(region, offs, out=out)
        finally:
            D.set_region_mode(0, mode)

    calls = {
        "rekey_same": lambda: M.rekey_dev(region, offs, rk["rekey_same"][1], aux, out=out, workspace=ws),
        "rekey_long": lambda: M.rekey_dev(region, offs, rk["rekey_long"][1], aux, out=out, workspace=ws),
        "transform": transform_general,
        "memcpy": lambda: hip.hipMemcpyAsync(out.data_ptr(), region.data_ptr(), region.numel(), 3, stream),
    }

    if only:  # a profiler run of some calls alone
        calls = {k: v for k, v in calls.items() if k in only}
        ref = next(iter(calls))
    else:
        ref = "rekey_same"

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
    assert "transform" not in calls or D.last_transform_path(0) == 0
    times = {name: [] for name in calls}
    for _ in range(reps):  # interleaved: every call sees the same machine state over the run
        for name in calls:
            times[name].append(once(name))
    ms = {name: sorted(t)[len(t) // 2] for name, t in times.items()}
    lo = {name: min(t) for name, t in times.items()}
    hi = {name: max(t) for name, t in times.items()}
    D.timing_enable(0, True)
    D.timing_collect_each(0)
    whole = once(ref)
    sweeps = D.timing_collect_each(0)
    D.timing_enable(0, False)
    if only:
        return {"case": f"rekey {m} x PUT({blob_bytes} B blob)", "messages": m, "region_bytes": m * L, "reps": reps,
                "ms_median": {k: round(x, 4) for k, x in ms.items()}, "timed_call": ref, "timed_call_ms": round(whole, 4),
                "timed_call_sweeps_ms": [round(x, 4) for x in sweeps]}
    return {"case": f"rekey {m} x PUT({blob_bytes} B blob)", "messages": m, "region_bytes": m * L, "reps": reps,
            "ms_median": {k: round(x, 4) for k, x in ms.items()}, "ms_min": {k: round(x, 4) for k, x in lo.items()},
            "ms_max": {k: round(x, 4) for k, x in hi.items()},
            "rekey_same_over_transform": round(ms["rekey_same"] / ms["transform"], 3),
            "rekey_long_over_rekey_same": round(ms["rekey_long"] / ms["rekey_same"], 3),
            "rekey_same_over_memcpy": round(ms["rekey_same"] / ms["memcpy"], 3),
            "transform_spread": round((hi["transform"] - lo["transform"]) / ms["transform"], 3),
            "memcpy_GBps": round(m * L / (ms["memcpy"] / 1e3) / 1e9, 1),
            "rekey_same_GBps_region": round(m * L / (ms["rekey_same"] / 1e3) / 1e9, 1),
            "timed_call_ms": round(whole, 4), "timed_call_sweeps_ms": [round(x, 4) for x in sweeps],
            "parity": "every message re-keyed, outputs clean under ambrycrc_verify_messages_dev, new keys in place"}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default="4k,64k", help="comma list of %s" % ",".join(CASES))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--only", default=None,
                    help="comma list of calls to time alone (rekey_same, rekey_long, transform, memcpy): a "
                         "profiler run; no ratios")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    import torch

    from ambry_amd import device as D

    if not torch.cuda.is_available():
        raise SystemExit("bench_rekey: needs a GPU (no CPU fallback for a timing)")
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
