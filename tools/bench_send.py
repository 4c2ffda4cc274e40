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

import bench_common as B

CASES = {"4k": (262144, 4096), "64k": (65536, 65536)}


def run(m, blob_bytes, reps, only=None):
    import numpy as np
    import torch

    from ambry_amd import device as D
    from ambry_amd import messages as M

    region, offs, L, fo, _ = B.stored_puts(m, blob_bytes)
    idx, p0 = np.arange(m, dtype=np.uint64), fo["props"]
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

    def send(flag):
        return lambda: M.send_messages_dev(region, offs, flag, out=out, workspace=ws)

    def memcpy(nbytes):
        return B.memcpy_call(out, region, nbytes)

    calls = {
        "send_blob": send(M.SEND_BLOB), "send_all": send(M.SEND_ALL), "send_info": send(M.SEND_BLOB_INFO),
        "transform": B.job_mode(lambda: M.transform_dev(region, offs, out=out)),
        "verify_jobs": B.job_mode(lambda: D.verify_messages(region, offs, want_end=False)),
        "memcpy_blob": memcpy(m * span["send_blob"][2]), "memcpy_all": memcpy(m * L),
        "memcpy_info": memcpy(m * span["send_info"][2]),
    }
    if only:  # a profiler run of some calls alone
        calls = {k: v for k, v in calls.items() if k in only}

    for name, last in (("transform", D.last_transform_path), ("verify_jobs", D.last_message_mode)):
        if name in calls:  # region mode off for the call: the general path, job mode
            calls[name]()
            torch.cuda.synchronize()
            assert last(0) == 0
    ms, lo, hi = B.time_interleaved(calls, reps)
    res = {"case": f"send {m} x PUT({blob_bytes} B blob)", "messages": m, "region_bytes": m * L, "reps": reps,
           "sent_bytes": {k: m * v[2] for k, v in span.items()},
           "ms_median": B.rounded(ms), "ms_min": B.rounded(lo), "ms_max": B.rounded(hi)}
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


if __name__ == "__main__":
    B.main("bench_send", __doc__, CASES, "4k,64k", 15, run)
