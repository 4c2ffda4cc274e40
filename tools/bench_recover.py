#!/usr/bin/env python3
"""Time of the device message chain (ambrycrc_chain_messages_dev) and of the device recovery
(ambrycrc_recover_messages_dev) over a region of m stored V3 PUTs with random fields and blobs (made by the
in-place serializer), against baselines timed in the same run, interleaved call by call (HIP events around each
call, median of --reps after a warm-up):

  chain          the device chain alone: candidate scan, compaction, link, doubling rounds, emit
  recover        chain + verify of every slot + MessageInfo
  verify         ambrycrc_verify_messages_dev with the offsets given (what recover adds the chain and the info to)
  readbw         the read roof over the same bytes (ambrycrc_debug_readbw_dev, the sweep's access shape)
  chain_host     ambrycrc_chain_messages_host over a host copy of the region (one call, wall clock)

`decoy`: a region whose 64 KiB blobs repeat `00 01`, every other byte a candidate the scan must validate.
Before anything is timed the device chain is asserted equal to the host chain, and the recovery to have
recovered every message. Prints one JSON line per case, with the shares of the chain, the verify and the info
kernels in the recover call. The shares of the launch groups inside the chain (scan, compaction, doubling
rounds) come from a kernel trace of the call alone, a run of its own:
  rocprofv3 --kernel-trace --stats -- python tools/bench_recover.py --cases 4k --only recover"""
from __future__ import annotations

import ctypes
import time

import bench_common as B

CASES = {"4k": ("4k", 262144, 4096, False), "1k": ("1k", 262144, 1024, False), "100": ("100", 262144, 100, False),
         "decoy": ("decoy", 4096, 65536, True)}


def build_region(m, blob_bytes, decoy):
    """m V3 PUTs back to back on the device: (region, message length)."""
    import numpy as np
    import torch

    from ambry_amd import messages as M

    region, _, L, fo, descs = B.stored_puts(m, blob_bytes, um_len=100)
    if decoy:  # written over the sealed blobs, then sealed again: the in-place serializer reads what is there
        b0 = fo["blob"]
        region.view(m, L)[:, b0:b0 + blob_bytes] = torch.tensor([0, 1], dtype=torch.uint8, device="cuda").repeat(
            blob_bytes // 2)
        M.serialize_dev(torch.from_numpy(descs.view(np.uint8).copy()).cuda(), region)
    return region, L


def run(name, m, blob_bytes, decoy, reps, only=None):
    import numpy as np
    import torch

    from ambry_amd import device as D
    from ambry_amd._lib import check, lib

    region, L = build_region(m, blob_bytes, decoy)
    n = region.numel()
    max_m = m
    want = np.arange(m, dtype=np.uint64) * np.uint64(L)
    offs = torch.from_numpy(want.view(np.int64).copy()).cuda()
    ws = torch.empty(D.recover_workspace_bytes(n, max_m), dtype=torch.uint8, device="cuda")
    chain_out = D.chain_messages(region, 0, max_m, workspace=ws)
    rec_out = D.recover_messages(region, 0, max_m, workspace=ws)
    torch.cuda.synchronize()

    # parity first: the device chain is the host chain, and recovery recovers every message
    host = region.cpu().numpy()
    t0 = time.perf_counter()
    host_offs = D.chain_messages_host(host, 0, max_m + 1)
    chain_host_ms = (time.perf_counter() - t0) * 1e3
    got = chain_out[0].cpu().numpy().view(np.uint64)
    assert len(host_offs) == m and np.array_equal(got, np.asarray(host_offs, dtype=np.uint64)), "device chain != host chain"
    assert np.array_equal(got, want)
    res = D.recover_result(chain_out[1])
    assert (int(res["chained"]), int(res["end_off"]), int(res["end_status"]), int(res["more"])) == (m, n, 0, 0)
    res = D.recover_result(rec_out[3])
    assert (int(res["recovered"]), int(res["end_off"]), int(res["end_status"])) == (m, n, 0)
    assert int(rec_out[2].abs().sum().item()) == 0
    info = rec_out[1].cpu().numpy().reshape(-1).view(D.MESSAGE_INFO)
    assert np.array_equal(info["msg_off"], want) and (info["size"] == L).all()
    del host

    rb_out = torch.empty(D.grid_size(0) * 1024 * 32, dtype=torch.int32, device="cuda")
    rb_bytes = n & ~((256 << 10) - 1)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    calls = {
        "chain": lambda: D.chain_messages(region, 0, max_m, workspace=ws, out=chain_out),
        "recover": lambda: D.recover_messages(region, 0, max_m, workspace=ws, out=rec_out),
        "verify": lambda: D.verify_messages(region, offs, want_end=False),
        "readbw": lambda: check(lib().ambrycrc_debug_readbw_dev(ctypes.c_void_p(region.data_ptr()), rb_bytes,
                                                                ctypes.c_void_p(rb_out.data_ptr()), 1, stream), "readbw"),
    }
    if only:  # a profiler run of some calls alone
        calls = {k: v for k, v in calls.items() if k in only}

    ms, lo, hi = B.time_interleaved(calls, reps)
    out = {"case": f"recover {name}: {m} x PUT({blob_bytes} B blob)", "messages": m, "region_bytes": n, "reps": reps,
           "launches_chain": 5 + (max(m - 1, 1).bit_length() + 1),
           "ms_median": B.rounded(ms), "ms_min": B.rounded(lo), "ms_max": B.rounded(hi), "chain_host_ms": round(chain_host_ms, 2)}
    if not only:
        out.update({
            "chain_GBps": round(n / (ms["chain"] / 1e3) / 1e9, 1), "readbw_GBps": round(rb_bytes / (ms["readbw"] / 1e3) / 1e9, 1),
            "chain_over_readbw": round(ms["chain"] / ms["readbw"], 2),
            "chain_host_over_chain": round(chain_host_ms / ms["chain"], 1),
            "recover_over_verify": round(ms["recover"] / ms["verify"], 2),
            "recover_over_host_chain_plus_verify": round(ms["recover"] / (chain_host_ms + ms["verify"]), 4),
            "share_chain": round(ms["chain"] / ms["recover"], 3), "share_verify": round(ms["verify"] / ms["recover"], 3),
            "share_info": round(max(ms["recover"] - ms["chain"] - ms["verify"], 0.0) / ms["recover"], 3),
            "parity": "device chain equal to the host chain; every message recovered with its offset and size"})
    return out


if __name__ == "__main__":
    B.main("bench_recover", __doc__, CASES, "4k,1k,100,decoy", 15, run)
