#!/usr/bin/env python3
"""Time of the GPU PutRequest ingest (ambrycrc_ingest_put_requests_dev) over a wire buffer of m V5 frames
(24-B blob ids, 94-B VERSION_5 properties, 100-B user metadata, no encryption key, random blobs), against
baselines timed in the same run, interleaved call by call (HIP events around each call, median of --reps after
a warm-up):

  ingest       the whole call: parse, every wire byte hashed once, verdict, placement, write, copy
  two_calls    what a caller could do before from the same buffer: ambrycrc_batch_dev over the wire spans (the
               wire CRC) plus ambrycrc_serialize_puts_dev in copy mode with host-prepared descriptors
               (d_fields = d_blobs = the wire buffer); every byte is hashed twice and nothing is parsed
  memcpy       one hipMemcpyAsync of the wire bytes

Before anything is timed the ingest's output is asserted equal, byte for byte, to the serialize route's, its
wire CRCs to the batch's, and every status 0. Prints one JSON line per case."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CASES = {"4k": (262144, 4096), "64k": (65536, 65536), "4m": (512, 4 << 20)}


def run(m, blob_bytes, reps, only=None):
    import numpy as np
    import torch

    from ambry_amd import device as D
    from ambry_amd import messages as M
    from bench_put import props94

    key_len, um_len = 24, 100
    props = props94()
    client = b"bench-client"
    head = struct.pack(">hhii", 0, 5, 1, len(client)) + client
    body_at = 8 + len(head)
    # offsets in the frame: blob id, properties, umSize, user metadata, blobType + encKeyLen, isCompressed + blobSize
    p_at = body_at + key_len
    us_at = p_at + len(props)
    um_at = us_at + 4
    t_at = um_at + um_len
    b_at = t_at + 2 + 2 + 1 + 8
    crc_at = b_at + blob_bytes
    F = crc_at + 8
    wire = torch.empty(m * F, dtype=torch.uint8, device="cuda")
    D.fill_random(wire[: (m * F) // 16 * 16], 3, 0)
    w2 = wire.view(m, F)
    put = lambda at, b: w2[:, at:at + len(b)].copy_(torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda())  # noqa: E731
    put(0, struct.pack(">q", F) + head)
    put(p_at, props)
    put(us_at, struct.pack(">i", um_len))
    put(t_at, struct.pack(">hhbq", 0, 0, 1, blob_bytes))
    idx = np.arange(m, dtype=np.int64)
    span_off = torch.from_numpy(idx * F + body_at).cuda()
    span_len = torch.full((m,), crc_at - body_at, dtype=torch.int64, device="cuda")
    crc = D.crc32_batch(wire, span_off, span_len)
    c = crc.to(torch.int64) & 0xFFFFFFFF
    w2[:, crc_at:crc_at + 4] = 0
    for k in range(4):
        w2[:, crc_at + 4 + k] = ((c >> (8 * (3 - k))) & 0xFF).to(torch.uint8)

    refs = np.zeros(m, dtype=M.PUT_REQUEST_REF_DTYPE)
    refs["off"], refs["key_len"] = idx * F, key_len
    refs_t = torch.from_numpy(refs.view(np.uint8).copy()).cuda()
    L, _ = M.layout(M.PutMessage(key=bytes(key_len), props=props, usermeta=bytes(um_len), blob=bytes(blob_bytes)))
    descs = np.zeros(m, dtype=M.PUT_DESC_DTYPE)
    u = idx.astype(np.uint64)
    descs["out_off"] = u * L
    descs["key_src"], descs["props_src"] = u * F + body_at, u * F + p_at
    descs["usermeta_src"], descs["blob_src"] = u * F + um_at, u * F + b_at
    descs["blob_len"] = blob_bytes
    descs["key_len"], descs["props_len"], descs["usermeta_len"] = key_len, len(props), um_len
    descs["enckey_len"], descs["compressed"], descs["header_version"] = -1, 1, 3
    descs_t = torch.from_numpy(descs.view(np.uint8).copy()).cuda()

    cap = M.ingest_out_bound(wire.numel(), m)
    out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    out2 = torch.empty(m * L, dtype=torch.uint8, device="cuda")
    ws = torch.empty(M.ingest_workspace_size(m), dtype=torch.uint8, device="cuda")

    # parity before any timing: the ingest's bytes are the serialize route's, its wire CRCs the batch's
    _, ooff, olen, _, wcrc, total, st = M.ingest_put_requests_dev(wire, refs_t, out=out, workspace=ws)
    M.serialize_dev(descs_t, out2, fields=wire, blobs=wire)
    torch.cuda.synchronize()
    assert int(st.abs().sum().item()) == 0
    assert int(total.item()) == m * L and bool((olen == L).all())
    assert bool(torch.equal(ooff, torch.arange(m, device="cuda") * L))
    assert bool(torch.equal(wcrc, crc))
    assert bool(torch.equal(out[: m * L], out2))

    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    crc_out = torch.empty(m, dtype=torch.int32, device="cuda")

    def two_calls():
        D.crc32_batch(wire, span_off, span_len, out=crc_out)
        M.serialize_dev(descs_t, out2, fields=wire, blobs=wire)

    calls = {
        "ingest": lambda: M.ingest_put_requests_dev(wire, refs_t, out=out, workspace=ws),
        "two_calls": two_calls,
        "memcpy": lambda: hip.hipMemcpyAsync(out.data_ptr(), wire.data_ptr(), wire.numel(), 3, stream),
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
    times = {name: [] for name in calls}
    for _ in range(reps):  # interleaved: every call sees the same machine state over the run
        for name in calls:
            times[name].append(once(name))
    ms = {name: sorted(t)[len(t) // 2] for name, t in times.items()}
    res = {"case": f"ingest {m} x PutRequest({blob_bytes} B blob)", "requests": m, "wire_bytes": m * F, "reps": reps,
           "ms_median": {k: round(x, 4) for k, x in ms.items()},
           "ms_min": {k: round(min(t), 4) for k, t in times.items()},
           "ms_max": {k: round(max(t), 4) for k, t in times.items()}}
    if not only:
        res.update({"ingest_over_two_calls": round(ms["ingest"] / ms["two_calls"], 3),
                    "ingest_over_memcpy": round(ms["ingest"] / ms["memcpy"], 3),
                    "memcpy_GBps": round(m * F / (ms["memcpy"] / 1e3) / 1e9, 1),
                    "ingest_GBps_wire": round(m * F / (ms["ingest"] / 1e3) / 1e9, 1),
                    "parity": "output equal to the serialize route's bytes, wire CRCs to the batch's, every status 0"})
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default="4k,64k,4m", help="comma list of %s" % ",".join(CASES))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--only", default=None,
                    help="comma list of calls to time alone (ingest, two_calls, memcpy): a profiler run; no ratios")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    import torch

    from ambry_amd import device as D

    if not torch.cuda.is_available():
        raise SystemExit("bench_ingest: needs a GPU (no CPU fallback for a timing)")
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
