#!/usr/bin/env python3
"""Throughput of the GPU write path (ambrycrc_serialize_puts_dev): m PUT
messages laid out in HBM with every CRC trailer filled. Every message has the C1 shape (V3
header, key, BlobProperties, 1000 B user metadata) and a blob of the given size; the fields and
blobs sit in their own HBM buffers (copy mode) or already in place (in-place mode). Prints one
JSON line per case: GiB/s of message bytes written, and the HBM bytes the step must move
(copy: fields+blobs read, message written, message read for the CRCs; in place: message read).
The first result is checked byte-exact against the host serializer on sampled messages and by
ambrycrc_verify_messages_dev on all of them."""
from __future__ import annotations

import argparse
import json
import os
import time

from bench_common import _props_tensor, props94, stored_puts, time_interleaved  # noqa: F401 (props94: re-export)


def run(m, blob_bytes, reps, in_place, um_len=1000, blob_shift=0):
    import numpy as np
    import torch

    from ambry_amd import device as D
    from ambry_amd.messages import PUT_DESC_DTYPE, PutMessage, layout, serialize_dev, serialize_host

    # blob content at message offset 40 + 24 + 104 + (um_len + 14) + 13: 1195 = 11 mod 16 for the
    # default 1000-B user metadata (the copy's stores then sit 11 B off the loads); --um-len 1005
    # aligns them
    key_len, props_len = 24, 94
    tmpl = PutMessage(key=bytes(key_len), props=bytes(props_len), usermeta=bytes(um_len), blob=bytes(blob_bytes))
    L, fo = layout(tmpl)
    stride = (L + 15) // 16 * 16
    fstride = key_len + props_len + um_len
    descs = np.zeros(m, dtype=PUT_DESC_DTYPE)
    idx = np.arange(m, dtype=np.uint64)
    descs["out_off"] = idx * stride
    descs["key_src"] = idx * fstride
    descs["props_src"] = idx * fstride + key_len
    descs["usermeta_src"] = idx * fstride + key_len + props_len
    descs["blob_src"] = idx * blob_bytes + blob_shift
    descs["blob_len"] = blob_bytes
    descs["key_len"], descs["props_len"], descs["usermeta_len"] = key_len, props_len, um_len
    descs["enckey_len"] = -1
    descs["header_version"] = 3
    d_desc = torch.from_numpy(descs.view(np.uint8).copy()).cuda()
    fields = torch.empty(m * fstride + 16, dtype=torch.uint8, device="cuda")
    blobs = torch.empty(max(1, m * blob_bytes + blob_shift), dtype=torch.uint8, device="cuda")
    D.fill_random(fields, 1, 0)
    D.fill_random(blobs, 2, 0)
    fields[: m * fstride].view(m, fstride)[:, key_len:key_len + props_len] = _props_tensor(torch)
    out = torch.zeros(m * stride, dtype=torch.uint8, device="cuda")
    serialize_dev(d_desc, out, fields, blobs)  # copy mode fills `out`; in-place mode then reuses its bytes
    torch.cuda.synchronize()
    # check: sampled messages against the host serializer, all of them by the GPU verify (not for the
    # timing-only probe builds of tools/ab_build.sh, whose CRCs are wrong by design)
    fh = fields.cpu().numpy().tobytes()
    probe = os.environ.get("AMBRYCRC_ALLOW_PROBE") == "1"
    for i in sorted({0, m // 2, m - 1}) if not probe else ():
        bl = blobs[i * blob_bytes + blob_shift:(i + 1) * blob_bytes + blob_shift].cpu().numpy().tobytes()
        o = i * fstride
        msg = PutMessage(key=fh[o:o + key_len], props=fh[o + key_len:o + key_len + props_len],
                         usermeta=fh[o + key_len + props_len:o + fstride], blob=bl)
        assert out[i * stride:i * stride + L].cpu().numpy().tobytes() == serialize_host(msg)[0], i
    offs = torch.from_numpy(descs["out_off"].astype(np.int64)).cuda()
    st, _ = D.verify_messages(out, offs, want_end=False)
    assert probe or int(st.abs().sum().item()) == 0

    def step():
        if in_place:
            serialize_dev(d_desc, out)
        else:
            serialize_dev(d_desc, out, fields, blobs)

    ms = time_interleaved({"step": step}, reps, warm_s=0.3)[0]["step"]
    msg_bytes = m * L
    # in place: one read of each message (the CRC pass); copy mode: the fields read once and the
    # message written once (the copy-through sweep CRCs what it copies)
    moved = msg_bytes if in_place else (m * (fstride + blob_bytes) + msg_bytes)
    return {"case": f"serialize {m} x PUT({blob_bytes} B blob)", "mode": "in_place" if in_place else "copy",
            "messages": m, "message_bytes": msg_bytes, "ms_median": round(ms, 4),
            "GiBps_messages": round(msg_bytes / (ms / 1e3) / 2**30, 1),
            "messages_per_s": round(m / (ms / 1e3)),
            "hbm_bytes_min": moved, "GBps_hbm_min": round(moved / (ms / 1e3) / 1e9, 1),
            "parity": "3 sampled messages byte-exact vs ambrycrc_serialize_put_host; all verify clean on the GPU"}


def run_transform(m, blob_bytes, reps, verdict="device"):
    """ValidatingTransformer (ambrycrc_transform_messages_dev) over a region of m stored V3 PUTs (made by
    the serializer), re-serialized at V3. A dense clean V3 region takes the one-pass fast path: the
    region kernel reads each message once, verifying it, and writes it once into the output; the
    CRCs are the verified input trailers."""
    import torch

    from ambry_amd import device as D
    from ambry_amd.messages import out_bound, transform_dev

    prev = D.set_transform_verdict(0, verdict == "host")
    region, offs, L, _, _ = stored_puts(m, blob_bytes)
    out = torch.empty(out_bound(m * L, m), dtype=torch.uint8, device="cuda")
    _, oo, ol, st = transform_dev(region, offs, out=out)
    torch.cuda.synchronize()
    assert int(st.abs().sum().item()) == 0 and bool(torch.equal(out[: m * L], region))  # V3 -> V3: identical
    ms = time_interleaved({"transform": lambda: transform_dev(region, offs, out=out)}, reps, warm_s=0.3)[0]["transform"]
    # back to back: `reps` calls between two events, one synchronize (a replication thread's pattern;
    # the side-stream verdict's chain of call k then overlaps call k + 1)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        transform_dev(region, offs, out=out)
    e1.record()
    torch.cuda.synchronize()
    ms_b2b = e0.elapsed_time(e1) / reps
    nbytes = m * L
    path = D.last_transform_path(0)
    D.set_transform_verdict(0, bool(prev))
    return {"case": f"transform {m} x PUT({blob_bytes} B blob) V3 -> V3", "verdict": verdict,
            "messages": m, "message_bytes": nbytes,
            "ms_median": round(ms, 4), "ms_back_to_back": round(ms_b2b, 4),
            "GiBps_messages": round(nbytes / (ms / 1e3) / 2**30, 1),
            "messages_per_s": round(m / (ms / 1e3)), "GBps_hbm_min": round(2 * nbytes / (ms / 1e3) / 1e9, 1),
            "parity": "every message verifies and the V3 -> V3 output equals the input region byte for byte",
            "path_taken": {1: "one-pass fast path", 0: "general path"}.get(path)}


def run_transform_host(m, blob_bytes, reps, leg="gpu", verdict="device", op="transform"):
    """ambrycrc_transform_messages_host over the same region in pageable host memory (the replication
    sieve's case: a GetResponse read into a heap or direct buffer), output into host memory: the GPU
    leg streams it through the pinned slabs (H2D, the fast path per slab, D2H), the CPU leg runs the
    per-message transform on the CPU threads. verdict=host is round 4's blocking per-slab verdict.
    Wall time per synchronous call, buffers preallocated."""
    import ctypes

    import numpy as np
    import torch

    from ambry_amd import device as D
    from ambry_amd._lib import check, lib
    from ambry_amd.messages import out_bound

    region, _, L, _, _ = stored_puts(m, blob_bytes)
    torch.cuda.synchronize()
    host = region.cpu().numpy()  # pageable
    del region
    offs = np.arange(m, dtype=np.uint64) * np.uint64(L)
    cap = out_bound(m * L, m)
    out = np.empty(cap, dtype=np.uint8)
    oo, ol = np.zeros(m, dtype=np.uint64), np.zeros(m, dtype=np.uint64)
    st = np.zeros(m, dtype=np.uint32)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    prev_policy = D.set_host_policy(0, D.HOST_GPU if leg == "gpu" else D.HOST_CPU)
    prev_verdict = D.set_transform_verdict(0, verdict == "host")

    def call():
        if op == "verify":
            check(lib().ambrycrc_verify_messages_host(
                ctypes.c_void_p(host.ctypes.data), host.size, offs.ctypes.data_as(u64p), m,
                st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), oo.ctypes.data_as(u64p), 0, 0),
                "ambrycrc_verify_messages_host")
            return
        check(lib().ambrycrc_transform_messages_host(
            ctypes.c_void_p(host.ctypes.data), host.size, offs.ctypes.data_as(u64p), m, None, 3, out.ctypes.data, cap,
            oo.ctypes.data_as(u64p), ol.ctypes.data_as(u64p), st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), 0, 0),
            "ambrycrc_transform_messages_host")

    try:
        call()
        if op == "verify":  # every message clean, each ending where the next starts
            assert int(st.max()) == 0 and np.array_equal(oo, offs + L)
        else:
            assert int(st.max()) == 0 and np.array_equal(out[: m * L], host)  # V3 -> V3: identical
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            call()
            times.append(time.perf_counter() - t0)
        path = D.last_host_path(0)
    finally:
        D.set_host_policy(0, prev_policy)
        D.set_transform_verdict(0, bool(prev_verdict))
    times.sort()
    ms = 1e3 * times[len(times) // 2]
    nbytes = m * L
    what = "verify_host" if op == "verify" else "transform_host"
    return {"case": f"{what} {m} x PUT({blob_bytes} B blob) V3 -> V3, pageable", "leg": leg,
            "verdict": verdict, "messages": m, "message_bytes": nbytes, "ms_median": round(ms, 3),
            "GiBps_messages": round(nbytes / (ms / 1e3) / 2**30, 2), "leg_taken": {0: "cpu", 1: "gpu"}.get(path),
            "parity": "every message verifies and the V3 -> V3 output equals the input region byte for byte"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cases", default="64k,4k,4m")
    ap.add_argument("--um-len", type=int, default=1000, help="user metadata bytes per PUT (1005: blob stores aligned)")
    ap.add_argument("--blob-shift", type=int, default=0,
                    help="blob source offset within its buffer (11 with the default user metadata: loads aligned)")
    ap.add_argument("--copy-only", action="store_true", help="skip the in-place mode")
    ap.add_argument("--transform", default="64k,4k,4m", help="ValidatingTransformer cases ('' for none)")
    ap.add_argument("--verdict", default="device,host",
                    help="how the transform learns its fast path's verdict: device (async, the default), host")
    ap.add_argument("--transform-host", default="", help="host-resident transform cases (pageable region, both legs)")
    args = ap.parse_args()
    import torch

    from ambry_amd import device as D

    torch.cuda.set_device(0)
    D.init(0)
    cases = {"64k": (65536, 64 << 10), "32k": (32768, 32 << 10), "16k": (65536, 16 << 10), "8k": (131072, 8 << 10),
             "4k": (262144, 4 << 10), "4m": (4096, 4 << 20),
             # the 4 KiB case at 4x and 16x the region (5.6 / 22 GB): where the copy plateaus
             "4kx4": (1048576, 4 << 10), "4kx16": (4194304, 4 << 10)}
    for c in [x for x in args.cases.split(",") if x]:
        m, s = cases[c]
        for in_place in (False, True):
            if in_place and args.copy_only:
                continue
            r = run(m, s, args.reps, in_place, args.um_len, args.blob_shift)
            r["usermeta_bytes"] = args.um_len
            r["blob_shift"] = args.blob_shift
            print(json.dumps(r), flush=True)
            torch.cuda.empty_cache()
    for c in [x for x in args.transform.split(",") if x]:
        m, s = cases[c]
        for v in [x for x in args.verdict.split(",") if x]:
            print(json.dumps(run_transform(m, s, args.reps, v)), flush=True)
            torch.cuda.empty_cache()
    for c in [x for x in args.transform_host.split(",") if x]:
        m, s = cases[c]
        for leg, v in (("gpu", "device"), ("gpu", "host"), ("cpu", "device")):
            print(json.dumps(run_transform_host(m, s, max(3, args.reps // 2), leg, v)), flush=True)
            torch.cuda.empty_cache()
        for leg in ("gpu", "cpu"):
            print(json.dumps(run_transform_host(m, s, max(3, args.reps // 2), leg, "device", op="verify")), flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
