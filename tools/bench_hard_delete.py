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

import ctypes

import bench_common as B

CASES = {"4k": (262144, 4096), "64k": (65536, 65536), "4m": (1024, 4 << 20)}


def run(m, blob_bytes, reps):
    import torch

    from ambry_amd import device as D

    um_len = 1000
    region, offs, L, fo, _ = B.stored_puts(m, blob_bytes, um_len=um_len)
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

    def restore(name):  # before every call that reads the records, outside the timed span
        if calls[name][0]:
            region.copy_(saved)

    ms, lo, _ = B.time_interleaved({k: v[1] for k, v in calls.items()}, reps, prepare=restore)
    return {"case": f"hard delete {m} x PUT({blob_bytes} B blob)", "messages": m, "region_bytes": m * L,
            "zeroed_bytes": zeroed, "reps": reps,
            "ms_median": B.rounded(ms), "ms_min": B.rounded(lo),
            "memset_GBps": round(zeroed / (ms["memset"] / 1e3) / 1e9, 1),
            "fill_call_GBps_zeroed": round(zeroed / (ms["fill"] / 1e3) / 1e9, 1),
            "fill_call_over_memset": round(ms["fill"] / ms["memset"], 3),
            "full_call_over_verify_plus_memset": round(ms["full"] / (ms["verify"] + ms["memset"]), 3),
            "verify_mode": D.last_message_mode(0),
            "parity": "every message deleted and clean under ambrycrc_verify_messages_dev, bodies zero, "
                      "bytes outside the two records unchanged"}


if __name__ == "__main__":
    B.main("bench_hard_delete", __doc__, CASES, "4k,64k,4m", 20, run, only=False)
