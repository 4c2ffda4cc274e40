"""What the feature benchmarks (bench_send, bench_recv, bench_rekey, bench_ingest, bench_hard_delete,
bench_recover, bench_put) share: the region of stored V3 PUTs they work on, the hipMemcpyAsync baseline, the
job-mode wrapper, the event-timed interleaved loop and the command line. The timing loop is the project's method
for "speed unchanged" (DESIGN.md §18.2, §20.2, §21): it lives here once."""
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


def props94() -> bytes:
    """94 bytes of valid BlobPropertiesSerDe V5 (BlobPropertiesSerDe.java:83-103): ttl -1, public,
    fixed creation time, contentType / ownerId / serviceId strings, account 101, container 5, not
    encrypted, three null strings. The message verify parses the properties (deserializeBlobAll),
    so the fields buffer must hold real ones, not random bytes."""
    out = struct.pack(">hqbqq", 5, -1, 0, 1_700_000_000_000, 4096)
    for s in (b"application/octet-stream", b"owner-01", b"svc001"):
        out += struct.pack(">i", len(s)) + s
    out += struct.pack(">hhb", 101, 5, 0) + struct.pack(">iii", 0, 0, 0)
    assert len(out) == 94
    return out


def _props_tensor(torch):
    import numpy as np

    return torch.from_numpy(np.frombuffer(props94(), dtype=np.uint8).copy()).cuda()


def stored_puts(m, blob_bytes, key_len=24, props_len=94, um_len=1000):
    """A region of m stored V3 PUTs back to back on the device, random fields and blobs under real properties,
    sealed by the in-place serializer: (region, offsets int64[m], message length L, {field: offset in the
    message}, the descriptor array)."""
    import numpy as np
    import torch

    from ambry_amd import device as D
    from ambry_amd import messages as M

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
    return region, torch.from_numpy((idx * L).astype(np.int64)).cuda(), L, fo, descs


def memcpy_call(dst, src, nbytes):
    """A call that enqueues one hipMemcpyAsync of nbytes from src to dst (tensors) on the current stream."""
    import torch

    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    return lambda: hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, stream)


def job_mode(fn):
    """fn with region mode off for the call: the verify in job mode, the transform on its general path."""
    from ambry_amd import device as D

    mode = D.get_region_mode(0)

    def call():
        D.set_region_mode(0, 0)
        try:
            fn()
        finally:
            D.set_region_mode(0, mode)
    return call


def time_interleaved(calls, reps, warm_s=0.5, prepare=None):
    """({name: median ms}, {name: min}, {name: max}) of `reps` rounds over calls ({name: function}), each call
    between two HIP events and followed by a synchronize, after warm_s seconds of such rounds. Interleaved: every
    call sees the same machine state over the run. prepare(name) runs before a call, outside its timed span."""
    import torch

    def once(name):
        if prepare:
            prepare(name)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        calls[name]()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    t_pre = time.perf_counter()
    while time.perf_counter() - t_pre < warm_s:
        for name in calls:
            once(name)
    times = {name: [] for name in calls}
    for _ in range(reps):
        for name in calls:
            times[name].append(once(name))
    return ({k: sorted(t)[len(t) // 2] for k, t in times.items()}, {k: min(t) for k, t in times.items()},
            {k: max(t) for k, t in times.items()})


def rounded(ms, digits=4):
    return {k: round(x, digits) for k, x in ms.items()}


def main(tool, doc, cases, default_cases, default_reps, run, only=True):
    """The tools' command line: run(*cases[name], reps[, only]) per case of --cases, one JSON line each."""
    ap = argparse.ArgumentParser(description=doc, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default=default_cases, help="comma list of %s" % ",".join(cases))
    ap.add_argument("--reps", type=int, default=default_reps)
    if only:
        ap.add_argument("--only", default=None, help="comma list of calls to time alone: a profiler run; no ratios")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    import torch

    from ambry_amd import device as D

    if not torch.cuda.is_available():
        raise SystemExit(f"{tool}: needs a GPU (no CPU fallback for a timing)")
    torch.cuda.set_device(0)
    D.init(0)
    for name in args.cases.split(","):
        extra = ((args.only.split(",") if args.only else None),) if only else ()
        line = json.dumps(run(*cases[name], args.reps, *extra))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        torch.cuda.empty_cache()
