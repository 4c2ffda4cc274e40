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

import struct

import bench_common as B

CASES = {"4k": (262144, 4096), "64k": (65536, 65536), "4m": (512, 4 << 20)}


def run(m, blob_bytes, reps, only=None):
    import numpy as np
    import torch

    from ambry_amd import device as D
    from ambry_amd import messages as M

    key_len, um_len = 24, 100
    props = B.props94()
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

    crc_out = torch.empty(m, dtype=torch.int32, device="cuda")

    def two_calls():
        D.crc32_batch(wire, span_off, span_len, out=crc_out)
        M.serialize_dev(descs_t, out2, fields=wire, blobs=wire)

    calls = {
        "ingest": lambda: M.ingest_put_requests_dev(wire, refs_t, out=out, workspace=ws),
        "two_calls": two_calls,
        "memcpy": B.memcpy_call(out, wire, wire.numel()),
    }
    if only:  # a profiler run of some calls alone
        calls = {k: v for k, v in calls.items() if k in only}

    ms, lo, hi = B.time_interleaved(calls, reps)
    res = {"case": f"ingest {m} x PutRequest({blob_bytes} B blob)", "requests": m, "wire_bytes": m * F, "reps": reps,
           "ms_median": B.rounded(ms), "ms_min": B.rounded(lo), "ms_max": B.rounded(hi)}
    if not only:
        res.update({"ingest_over_two_calls": round(ms["ingest"] / ms["two_calls"], 3),
                    "ingest_over_memcpy": round(ms["ingest"] / ms["memcpy"], 3),
                    "memcpy_GBps": round(m * F / (ms["memcpy"] / 1e3) / 1e9, 1),
                    "ingest_GBps_wire": round(m * F / (ms["ingest"] / 1e3) / 1e9, 1),
                    "parity": "output equal to the serialize route's bytes, wire CRCs to the batch's, every status 0"})
    return res


if __name__ == "__main__":
    B.main("bench_ingest", __doc__, CASES, "4k,64k,4m", 15, run)
