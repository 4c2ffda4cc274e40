#!/usr/bin/env python3
"""Time of the GPU GET receive (ambrycrc_receive_blobs_dev) over the body ambrycrc_send_messages_dev produces from a
region of m stored V3 PUTs with random fields and blobs (made by the in-place serializer), against baselines timed
in the same run, interleaved call by call (HIP events around each call, median of --reps after a warm-up):

  recv_blob        BLOB, packed: every blob record's content delivered back to back
  recv_blob_range  BLOB with a range on every payload ([100, size - 100)): three CRC jobs a payload, not one
  recv_all         ALL over the stored messages themselves (what send's ALL emits): the verify's parse and three
                   more records a payload hashed
  send_blob        ambrycrc_send_messages_dev(BLOB) over the stored messages the records came from: it reads and
                   writes the same bytes as recv_blob, which should be no slower than it -- the allowance is send's
                   own spread (max - min) in this run
  verify_jobs      ambrycrc_verify_messages_dev in job mode: the read and the hash without the write
  memcpy           one hipMemcpyAsync of the delivered bytes

The first receive of each kind is checked: every payload clean, slices packed back to back, and the output equal to
the stored content. Prints one JSON line per case."""
from __future__ import annotations

import bench_common as B

CASES = {"4k": (262144, 4096), "64k": (65536, 65536), "4m": (2048, 4 << 20)}


def run(m, blob_bytes, reps, only=None):
    import numpy as np
    import torch

    from ambry_amd import device as D
    from ambry_amd import messages as M

    region, offs, L, fo, _ = B.stored_puts(m, blob_bytes)
    idx = np.arange(m, dtype=np.uint64)
    sizes_all = torch.full((m,), L, dtype=torch.int64, device="cuda")
    blob_rel, rec = fo["blob"] - 13, L - (fo["blob"] - 13)  # the blob record: 13-B head, content, 8-B CRC
    body = torch.empty(m * rec, dtype=torch.uint8, device="cuda")
    send_ws = torch.empty(M.send_workspace_bytes(m), dtype=torch.uint8, device="cuda")
    _, sinfo, sst = M.send_messages_dev(region, offs, M.SEND_BLOB, out=body, workspace=send_ws)
    torch.cuda.synchronize()
    assert int(sst.abs().sum().item()) == 0
    sf = sinfo.cpu().numpy().view(M.SEND_INFO_DTYPE)
    pay_off = torch.from_numpy(sf["out_off"].astype(np.int64)).cuda()
    pay_size = torch.from_numpy(sf["send_len"].astype(np.int64)).cuda()
    lo, hi = 100, blob_bytes - 100
    ranges = torch.tensor([lo, hi], dtype=torch.int64, device="cuda").repeat(m)
    out = torch.empty(m * blob_bytes, dtype=torch.uint8, device="cuda")
    ws = torch.empty(M.receive_workspace_bytes(m), dtype=torch.uint8, device="cuda")
    content = region.view(m, L)[:, fo["blob"]:fo["blob"] + blob_bytes]

    kinds = {"recv_blob": (body, pay_off, pay_size, M.SEND_BLOB, None, 0, blob_bytes),
             "recv_blob_range": (body, pay_off, pay_size, M.SEND_BLOB, ranges, lo, hi),
             "recv_all": (region, offs, sizes_all, M.SEND_ALL, None, 0, blob_bytes)}

    def recv(name):
        b, po, ps, flag, rg, _, _ = kinds[name]
        return lambda: M.receive_blobs_dev(b, po, flag, pay_size=ps, ranges=rg, out=out, workspace=ws)

    for name, (_, _, _, flag, _, a, z) in kinds.items():  # a check of the whole pipeline once per kind
        out.fill_(0)
        _, info, st = recv(name)()
        torch.cuda.synchronize()
        assert int(st.abs().sum().item()) == 0, name
        f = info.cpu().numpy().view(M.RECV_INFO_DTYPE)
        n = z - a
        assert (f["out_len"] == n).all() and (f["blob_size"] == blob_bytes).all(), name
        assert (f["out_off"] == idx * np.uint64(n)).all(), name
        assert bool(torch.equal(out[: m * n].view(m, n), content[:, a:z])), name

    sent = torch.empty(m * rec, dtype=torch.uint8, device="cuda")
    calls = {name: recv(name) for name in kinds}
    calls.update({
        "send_blob": lambda: M.send_messages_dev(region, offs, M.SEND_BLOB, out=sent, workspace=send_ws),
        "verify_jobs": B.job_mode(lambda: D.verify_messages(region, offs, want_end=False)),
        "memcpy": B.memcpy_call(out, body, m * blob_bytes),
    })
    if only:  # a profiler run of some calls alone
        calls = {k: v for k, v in calls.items() if k in only}

    if "verify_jobs" in calls:
        calls["verify_jobs"]()
        torch.cuda.synchronize()
        assert D.last_message_mode(0) == 0
    ms, lo_t, hi_t = B.time_interleaved(calls, reps)
    res = {"case": f"recv {m} x blob record({blob_bytes} B)", "payloads": m, "body_bytes": m * rec,
           "delivered_bytes": m * blob_bytes, "reps": reps,
           "ms_median": B.rounded(ms), "ms_min": B.rounded(lo_t), "ms_max": B.rounded(hi_t)}
    if not only:
        allowance = hi_t["send_blob"] - lo_t["send_blob"]
        res.update({
            "recv_blob_over_send_blob": round(ms["recv_blob"] / ms["send_blob"], 3),
            "send_blob_spread_ms": round(allowance, 4),
            "recv_blob_within_send_spread": bool(ms["recv_blob"] <= ms["send_blob"] + allowance),
            "recv_blob_range_over_recv_blob": round(ms["recv_blob_range"] / ms["recv_blob"], 3),
            "recv_all_over_recv_blob": round(ms["recv_all"] / ms["recv_blob"], 3),
            "recv_blob_over_verify_jobs": round(ms["recv_blob"] / ms["verify_jobs"], 3),
            "recv_blob_over_memcpy": round(ms["recv_blob"] / ms["memcpy"], 3),
            "recv_blob_GBps_delivered": round(m * blob_bytes / (ms["recv_blob"] / 1e3) / 1e9, 1),
            "parity": "every payload clean, slices packed, output equal to the stored content"})
    return res


if __name__ == "__main__":
    B.main("bench_recv", __doc__, CASES, "4k,64k,4m", 21, run)
