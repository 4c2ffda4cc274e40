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

import bench_common as B

CASES = {"4k": (262144, 4096), "64k": (65536, 65536)}


def run(m, blob_bytes, reps, only=None):
    import numpy as np
    import torch

    from ambry_amd import device as D
    from ambry_amd import messages as M

    key_len = 24
    region, offs, L, _, _ = B.stored_puts(m, blob_bytes, key_len)
    idx = np.arange(m, dtype=np.uint64)

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

    calls = {
        "rekey_same": lambda: M.rekey_dev(region, offs, rk["rekey_same"][1], aux, out=out, workspace=ws),
        "rekey_long": lambda: M.rekey_dev(region, offs, rk["rekey_long"][1], aux, out=out, workspace=ws),
        "transform": B.job_mode(lambda: M.transform_dev(region, offs, out=out)),  # verify jobs, layout, seal
        "memcpy": B.memcpy_call(out, region, region.numel()),
    }

    if only:  # a profiler run of some calls alone
        calls = {k: v for k, v in calls.items() if k in only}
        ref = next(iter(calls))
    else:
        ref = "rekey_same"

    if "transform" in calls:
        calls["transform"]()
        torch.cuda.synchronize()
        assert D.last_transform_path(0) == 0
    ms, lo, hi = B.time_interleaved(calls, reps)
    D.timing_enable(0, True)
    D.timing_collect_each(0)
    whole = B.time_interleaved({ref: calls[ref]}, 1, warm_s=0)[0][ref]
    sweeps = D.timing_collect_each(0)
    D.timing_enable(0, False)
    if only:
        return {"case": f"rekey {m} x PUT({blob_bytes} B blob)", "messages": m, "region_bytes": m * L, "reps": reps,
                "ms_median": B.rounded(ms), "timed_call": ref, "timed_call_ms": round(whole, 4),
                "timed_call_sweeps_ms": [round(x, 4) for x in sweeps]}
    return {"case": f"rekey {m} x PUT({blob_bytes} B blob)", "messages": m, "region_bytes": m * L, "reps": reps,
            "ms_median": B.rounded(ms), "ms_min": B.rounded(lo), "ms_max": B.rounded(hi),
            "rekey_same_over_transform": round(ms["rekey_same"] / ms["transform"], 3),
            "rekey_long_over_rekey_same": round(ms["rekey_long"] / ms["rekey_same"], 3),
            "rekey_same_over_memcpy": round(ms["rekey_same"] / ms["memcpy"], 3),
            "transform_spread": round((hi["transform"] - lo["transform"]) / ms["transform"], 3),
            "memcpy_GBps": round(m * L / (ms["memcpy"] / 1e3) / 1e9, 1),
            "rekey_same_GBps_region": round(m * L / (ms["rekey_same"] / 1e3) / 1e9, 1),
            "timed_call_ms": round(whole, 4), "timed_call_sweeps_ms": [round(x, 4) for x in sweeps],
            "parity": "every message re-keyed, outputs clean under ambrycrc_verify_messages_dev, new keys in place"}


if __name__ == "__main__":
    B.main("bench_rekey", __doc__, CASES, "4k,64k", 15, run)
