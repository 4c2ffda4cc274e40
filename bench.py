#!/usr/bin/env python3
"""bench.py -- device-resident CRC-32 over 4 MiB blob chunks (BASELINE.json metric).

One step = one pass of the hot path over one batch resident in HBM on every GPU:
  N = 1  config C3 (8,192 x 4 MiB = 32 GiB): ambrycrc_batch_dev (plan + sweep kernels).
  N > 1  config C5's per-GPU shard (65,536 x 4 MiB = 256 GiB per GPU; C5 = 524,288 chunks on
         8 GPUs): every GPU CRCs its shard, then one RCCL all-gather of the 4-byte CRCs over
         xGMI leaves the whole batch's CRCs on every GPU -- both inside libambrycrc's C ABI:
           WORLD_SIZE set (torchrun, one process per GPU): ambrycrc_batch_dev_gather on a
             communicator built from ambrycrc_unique_id (sent over a gloo control group);
           WORLD_SIZE unset, --gpus N: one process drives N GPUs, ambrycrc_batch_dev_multi.
         Weak scaling: the per-GPU shard is fixed as N grows.
  --config c1   one 64 KiB PUT message on the CPU (BASELINE configs[0]): µs per message for the
                product host path and for the oracle; not the headline metric.

A plain run sets up, warms up, times --steps steps, writes the last step's outputs if
--dump-outputs is given, and prints ONE JSON line (rank 0). Besides the driver contract it carries:
  roofline      sweep-kernel algorithmic bytes / its HIP-event-timed duration (events recorded
                inside the timed steps) vs 8 TB/s; traffic from bench_data/pmc_traffic.json
                (rocprofv3 PMC, (2*FETCH_SIZE+WRITE_SIZE) KiB)
--full adds the legs that take runs of their own, after the timed steps:
  roofline.measured_read_roof   the read-only probe over the same buffer
  cpu_baseline  the oracle's restatement of Crc32.java (kind "port") on host cores, 1 thread and
                the process's CPU share, over a DRAM-resident sample (> L3)
  host_path     pinned-host -> HBM -> CRC rate (PCIe-inclusive; never `value`)
  rccl          N > 1: ranks RCCL saw and whether every GPU's gathered vector is right
  verify        c4: whether the flags name exactly the flipped chunks

--dump-outputs DIR writes what the last timed step left for its caller as DIR/<name>.npy
(float64, so every 32-bit CRC is exact): crc32 (one GPU), mismatch beside it (c4), or
gathered_crc32 (N > 1 and the RCCL forms). The workload is seeded, so two builds can be compared
output for output.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import resource
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

METRIC = "GiB/s device-resident CRC32 over 4 MiB blob chunks; % of HBM roofline"
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s (spec)
TRAFFIC_FILE = os.path.join(ROOT, "bench_data", "pmc_traffic.json")

CONFIGS = {
    # name: (chunks per GPU, chunk bytes, description)
    "c3": (8192, 4 << 20, "C3: 8,192 x 4 MiB large-blob router chunks per GPU"),
    "c2": (65536, 64 << 10, "C2: 65,536 x 64 KiB small-object chunks per GPU"),
    # 524,288 x 4 MiB over 8 GPUs = 65,536 x 4 MiB = 256 GiB resident per
    # GPU (of 268 GiB HBM). Every chunk is distinct: a reused buffer let waves that run at
    # the same time read the same bytes, and the caches then served ~4 % of the reads.
    "c5": (65536, 4 << 20, "C5: 65,536 x 4 MiB chunks per GPU (256 GiB resident; 524,288 on 8 GPUs)"),
}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default=None, choices=sorted(CONFIGS) + ["c1", "c4"],
                    help="default: c3 at one GPU, c5 (per-GPU shard) at N > 1")
    ap.add_argument("--variant", type=int, default=None)
    ap.add_argument("--grid", type=int, default=None, help="sweep-kernel workgroups (default: one per CU)")
    ap.add_argument("--window", type=int, default=None,
                    help="sweep rounds of at most this many bytes (default: the library's 32 GiB; 0 = one round)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also run the legs that take runs of their own: read-roof "
                         "probe, CPU baseline, host-resident path, RCCL gather check, c4 flag check")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs as DIR/<name>.npy (float64)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-host-path", action="store_true", help="with --full: skip the host-resident path")
    ap.add_argument("--cpu-seconds", type=float, default=10.0)
    ap.add_argument("--cpu-sample-gib", type=float, default=2.0,
                    help="CPU baseline sample (GiB): several times the host's L3, so it is a DRAM rate")
    ap.add_argument("--prewarm-s", type=float, default=0.3, help="untimed clock-ramp run before warmup")
    ap.add_argument("--quiet", action="store_true", help="no progress lines on stderr")
    ap.add_argument("--force-dist", action="store_true",
                    help="one-process-per-GPU form even at WORLD_SIZE=1 (gloo control group + RCCL gather)")
    ap.add_argument("--inproc", action="store_true",
                    help="one-process multi-GPU form (ambrycrc_batch_dev_multi) even at --gpus 1")
    return ap.parse_args()


def log(args, *msg):
    if not args.quiet:
        print("[bench]", *msg, file=sys.stderr, flush=True)


def build_workload(torch, dev, config, seed_rank):
    """One GPU's batch in HBM: (buf, off, len, n, total bytes, chunk bytes or None, description)."""
    import numpy as np

    from ambry_amd import device as D

    if config == "c4":
        from datagen import zipf_sizes

        sizes = zipf_sizes(32768)
        off = [0]
        for s in sizes[:-1]:
            off.append(off[-1] + ((int(s) + 15) // 16) * 16)
        total = off[-1] + int(sizes[-1])
        off_t = torch.tensor(np.asarray(off, dtype=np.int64), device=dev)
        len_t = torch.tensor(sizes.astype(np.int64), device=dev)
        desc = "C4: 32,768 Zipf(1.2) chunks 4 KiB-4 MiB (verify-on-read sizes)"
        n = len(sizes)
        chunk = None
    else:
        n, chunk, desc = CONFIGS[config]
        total = n * chunk
        off_t = torch.arange(n, dtype=torch.int64, device=dev) * chunk
        len_t = torch.full((n,), chunk, dtype=torch.int64, device=dev)
    buf = torch.empty(total, dtype=torch.uint8, device=dev)
    D.fill_random(buf, 0xA3B1C2D3 ^ (seed_rank * 0x9E3779B97F4A7C15 & (2**64 - 1)), 0)
    torch.cuda.synchronize(dev)
    return buf, off_t, len_t, n, total, chunk, desc


# ------------------------------------------------------------------ CPU baseline

def cpu_topology():
    """CPUs this process may use: affinity set, cgroup quota, physical cores behind the set."""
    aff = sorted(os.sched_getaffinity(0))
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, period = f.read().split()
            if q != "max":
                quota = max(1, int(int(q) // int(period)))
    except (OSError, ValueError):
        pass
    cores = set()
    for c in aff:
        try:
            with open(f"/sys/devices/system/cpu/cpu{c}/topology/core_id") as f:
                core = f.read().strip()
            with open(f"/sys/devices/system/cpu/cpu{c}/topology/physical_package_id") as f:
                pkg = f.read().strip()
            cores.add((pkg, core))
        except OSError:
            cores.add(("?", c))
    model = None
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    usable = min(len(aff), quota) if quota else len(aff)
    return {"cpu_model": model, "affinity_cpus": len(aff), "physical_cores_in_affinity": len(cores),
            "cgroup_cpu_quota": quota, "usable_cpus": usable, "nproc": os.cpu_count()}


def _timed(fn, nbytes, seconds):
    """Repeat fn() for about `seconds`; GiB/s, passes, last result."""
    t0 = time.perf_counter()
    passes = 0
    while True:
        out = fn()
        passes += 1
        el = time.perf_counter() - t0
        if el >= seconds or passes >= 1000:
            return passes * nbytes / el / 2**30, passes, out


def cpu_baseline(buf, off_t, len_t, n, args):
    """The oracle (oracle/crc32_ref.c: C restatement of Crc32.java's slice-by-8, kind "port") on
    the GPU box's host cores, over a sample of the same workload copied to host memory: at least
    --cpu-sample-gib (default 2 GiB, several times the host's L3), so the rate is a DRAM rate.
    1 thread, and the process's whole CPU share (min(affinity set, cgroup quota)); system zlib
    (java.util.zip.CRC32's function) and the library's own CLMUL loop beside it."""
    import numpy as np

    from conftest import ORACLE_SO, Oracle

    if not os.path.exists(ORACLE_SO):
        return None
    orc = Oracle()
    import ambry_amd
    from ambry_amd import device as D

    ln_all = len_t.cpu().numpy()
    want = int(args.cpu_sample_gib * 2**30)
    cum = np.cumsum(ln_all)
    k = int(min(n, np.searchsorted(cum, want) + 1))
    off = off_t[:k].cpu().numpy()
    ln = ln_all[:k]
    lo, hi = int(off[0]), int(off[-1] + ln[-1])
    host = buf[lo:hi].cpu().numpy()
    off = off - lo
    nbytes = int(ln.sum())
    topo = cpu_topology()
    share = topo["usable_cpus"]
    each = args.cpu_seconds / 7
    res = {}
    for zl in (False, True):
        for th in (1, share):
            res[(zl, th)] = _timed(lambda: orc.batch(host, off, ln, threads=th, zlib=zl), nbytes, each)
    assert np.array_equal(res[(True, share)][2], res[(False, share)][2]), "zlib vs restatement"
    gibs, passes, out = res[(False, share)]
    aff_run = None
    if topo["affinity_cpus"] > share:  # the whole affinity set, throttled to the quota by the cgroup
        aff_run = round(_timed(lambda: orc.batch(host, off, ln, threads=topo["affinity_cpus"]), nbytes, each)[0], 3)
    base = host.ctypes.data
    chunks = [(base + int(o), int(x)) for o, x in zip(off, ln)]
    clmul_out = np.asarray(D.crc32_batch_cpu(chunks, threads=1), dtype=np.uint32)
    clmul = {
        "impl": ambry_amd.lib().ambrycrc_host_impl().decode(),
        "single_thread_gibs": round(_timed(lambda: D.crc32_batch_cpu(chunks, threads=1), nbytes, each)[0], 3),
        "gibs": round(_timed(lambda: D.crc32_batch_cpu(chunks, threads=share), nbytes, each)[0], 3),
        "cores": share, "parity_vs_port": bool(np.array_equal(clmul_out, out)),
        "what": "libambrycrc ambrycrc_batch_cpu (CLMUL fold, the class of HotSpot's CRC32 intrinsic), same sample",
    }
    return {
        "value": round(gibs, 3), "unit": "GiB/s", "cores": share, "kind": "port",
        **topo,
        "sample": f"{k} chunks = {nbytes / 2**30:.2f} GiB (first chunks of the same workload, D2H-copied; "
                  f"> the host L3) x {passes} passes; oracle/crc32_ref.c slice-by-8 restating Crc32.java:55-98, "
                  f"{share} pthreads = the process's CPU share (cgroup quota {topo['cgroup_cpu_quota']}, "
                  f"affinity {topo['affinity_cpus']} CPUs)",
        "single_thread_gibs": round(res[(False, 1)][0], 3),
        "all_affinity_threads_gibs": aff_run,
        "zlib": {"gibs": round(res[(True, share)][0], 3), "cores": share,
                 "single_thread_gibs": round(res[(True, 1)][0], 3),
                 "what": "system zlib 1.2.11 crc32_z (the function java.util.zip.CRC32 wraps), same sample"},
        "host_clmul": clmul,
        "_out": out,
    }


# ------------------------------------------------------------------ probes

def measure_read_roof(torch, D, buf, total, device):
    """Read-only probe (ambrycrc_debug_readbw_dev variant 1: the sweep kernel's grid and access
    shape, nontemporal loads, no CRC arithmetic) over the same HBM buffer: best of 5 launches, GB/s."""
    from ambry_amd._lib import check, lib

    nbytes = total & ~((256 << 10) - 1)
    scratch = torch.empty(D.grid_size(device) * 1024, dtype=torch.int32, device=buf.device)
    best = None
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        check(lib().ambrycrc_debug_readbw_dev(buf.data_ptr(), nbytes, scratch.data_ptr(), 1,
                                              torch.cuda.current_stream().cuda_stream), "readbw")
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        best = ms if best is None else min(best, ms)
    return round(nbytes / (best / 1e3) / 1e9, 1)


def host_path_rate(torch, args):
    """Host buffers -> PCIe -> HBM -> CRC -> host (ambrycrc_batch_host); DESIGN.md only, never `value`.

    After one untimed full pass (first touch of the pinned pages by the DMA engine), the best
    of 3 synchronous calls for pinned and for pageable sources, beside the PCIe H2D roof: one
    2 GiB pinned->HBM hipMemcpyAsync (torch copy_) timed the same way.
    """
    from ambry_amd import device as D

    nchunks, chunk = 512, 4 << 20  # 2 GiB
    total = nchunks * chunk
    host = torch.empty(total, dtype=torch.uint8).pin_memory()
    host.view(torch.int64).random_()
    pageable = host.numpy().copy()

    cpu_cost = {}

    def best_of(fn, reps=3, name=None):
        """Best-of-reps GiB/s; with `name`, also this process's CPU-seconds per GiB over the reps
        (getrusage user + system: the CPU leg's threads, or the GPU leg's staging copies and waits)."""
        fn()
        best = None
        r0 = resource.getrusage(resource.RUSAGE_SELF)
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
            best = el if best is None else min(best, el)
        r1 = resource.getrusage(resource.RUSAGE_SELF)
        if name:
            cpu_s = (r1.ru_utime - r0.ru_utime) + (r1.ru_stime - r0.ru_stime)
            cpu_cost[name] = round(cpu_s / (reps * total / 2**30), 4)
        return total / best / 2**30

    # the CPU leg's calibration at its default budget, at a quiet moment: after the CPU baseline's threads,
    # a pause of a few cgroup quota periods (the box's CPU share is a CFS quota, which that leg exhausts)
    time.sleep(0.3)
    calib = D.host_calibrate(0)
    dev = torch.empty(total, dtype=torch.uint8, device="cuda")
    roof = best_of(lambda: dev.copy_(host, non_blocking=True))
    del dev
    res = {}
    prev = D.set_host_policy(0, D.HOST_GPU)  # the GPU leg itself, whatever auto would pick
    try:
        for name, base in (("pinned", host.data_ptr()), ("pageable", pageable.ctypes.data)):
            chunks = [(base + i * chunk, chunk) for i in range(nchunks)]
            res[name] = best_of(lambda: D.crc32_batch_host(chunks, device=0, pinned=name == "pinned"),
                                name="gpu_leg_" + name)
        # the CPU leg on the same pageable sample at its default budget (half the CPU share) and at the
        # whole share, and the leg the default (auto) policy takes at the default budget
        D.set_host_policy(0, D.HOST_CPU)
        chunks = [(pageable.ctypes.data + i * chunk, chunk) for i in range(nchunks)]
        res["cpu_leg"] = best_of(lambda: D.crc32_batch_host(chunks, device=0), name="cpu_leg_budget")
        budget = D.host_rates(0)["cpu_threads"]
        share = D.set_host_cpu_threads(0, 0) or 0  # (0: it was the default)
        D.set_host_cpu_threads(0, max(1, 2 * budget))
        res["cpu_leg_share"] = best_of(lambda: D.crc32_batch_host(chunks, device=0), name="cpu_leg_share")
        D.set_host_cpu_threads(0, share)
        D.set_host_policy(0, D.HOST_AUTO)
        res["auto"] = best_of(lambda: D.crc32_batch_host(chunks, device=0))
        auto_leg = "gpu" if D.last_host_path(0) == 1 else "cpu"
        rates = D.host_rates(0)
    finally:
        D.set_host_policy(0, prev)
    return {"value": round(res["pinned"], 2), "unit": "GiB/s",
            "pageable": round(res["pageable"], 2),
            "h2d_copy_roof": round(roof, 2),
            "frac_of_h2d_roof": round(res["pinned"] / roof, 4),
            "dispatch": {"cpu_leg_pageable": round(res["cpu_leg"], 2), "auto_pageable": round(res["auto"], 2),
                         "auto_leg": auto_leg, "cpu_threads": rates["cpu_threads"],
                         "cpu_leg_pageable_2x_threads": round(res["cpu_leg_share"], 2),
                         "policy_cpu_estimate": round(rates["cpu_gibps"], 1),
                         "cpu_calibration_at_budget": round(calib, 1),
                         "policy_gpu_estimate": round(rates["gpu_gibps"], 1),
                         "host_cpu_s_per_gib": cpu_cost},
            "sample": f"{nchunks} x 4 MiB host chunks (2 GiB), synchronous ambrycrc_batch_host (H2D + kernels + "
                      "D2H of CRCs), best of 3 after one untimed pass; pinned = hipHostMalloc'd source, "
                      "pageable = malloc'd source staged by the library's copy threads"}


def traffic_for(config):
    """rocprofv3 PMC traffic per sweep launch for this config, if one was collected (bench_data/)."""
    try:
        with open(TRAFFIC_FILE) as f:
            p = json.load(f).get(config)
    except (OSError, ValueError):
        return None, None
    if not p:
        return None, None
    return p.get("hbm_bytes_per_launch"), p.get("source")


def dump_outputs(path, arrays):
    """Each tensor the timed path handed back, as path/<name>.npy in float64 (exact for 32-bit CRCs)."""
    import numpy as np

    os.makedirs(path, exist_ok=True)
    for name, t in arrays.items():
        a = t.cpu().numpy()
        if a.dtype == np.int32:
            a = a.view(np.uint32)
        np.save(os.path.join(path, name + ".npy"), a.astype(np.float64))


# ------------------------------------------------------------------ C1 (CPU, one message)

def run_c1(args, result_fd):
    """BASELINE configs[0]: one 64 KiB-blob PUT message (V3 header, MockId("id1") key, BlobProperties,
    1000 B user metadata, blob record) through messageformat on the CPU.
      product (write)   ambrycrc_serialize_put_host: the whole message laid out and every CRC
                        trailer filled (PutMessageFormatInputStream + MessageFormatInputStream.read*,
                        PutMessageFormatInputStream.java:76-124); must equal the fixture's bytes
      product (verify)  ambrycrc_update per record, the blob record's CRC derived from the blob's
                        by ambrycrc_put_crcs (PutMessageFormatInputStream.java:116-120)
      product (read)    ambrycrc_verify_message_cpu: deserializeBlobAll's checks on the whole
                        message in one call (header, record versions / sizes, every CRC)
      cpu_baseline      the oracle's Crc32.java restatement over the same four records
    All checked against the committed fixture (tests/golden/c1_message.*)."""
    import ctypes

    import numpy as np

    from ambry_amd import lib
    from ambry_amd.messages import PutMessage
    from c1_message import c1_fixture, c1_message_bytes, c1_record_ranges
    from conftest import Oracle

    fx = c1_fixture()
    msg = c1_message_bytes()
    ranges = c1_record_ranges()
    L = lib()
    arr = np.frombuffer(msg, dtype=np.uint8)
    base = arr.ctypes.data
    expect = [int(x, 16) for x in fx["record_crcs"]]

    # write side: the C1 fields (sliced from the fixture) serialized by the product
    ko, kl = fx["key_offset"], fx["key_bytes"]
    (p0, p1), (u0, u1), (b0, b1) = ranges[1], ranges[2], ranges[3]
    m = PutMessage(key=msg[ko:ko + kl], props=msg[p0 + 2:p1], usermeta=msg[u0 + 6:u1], blob=msg[b0 + 13:b1])
    fields = m.key + m.props + m.usermeta
    src = {"key": 0, "props": len(m.key), "usermeta": len(m.key) + len(m.props), "blob": 0}
    desc = m.desc(0, src)
    fbuf = ctypes.create_string_buffer(fields, len(fields))
    bbuf = ctypes.create_string_buffer(m.blob, len(m.blob))
    out = ctypes.create_string_buffer(len(msg))
    crcs = (ctypes.c_uint32 * 5)()
    dref = ctypes.byref(desc)

    def write():
        L.ambrycrc_serialize_put_host(dref, fbuf, bbuf, out, len(msg), crcs)

    write()
    ok_w = out.raw == msg and [crcs[0], crcs[2], crcs[3], crcs[4]] == expect

    bl0, bl1 = ranges[-1]  # blob record: 13-B prefix + content
    content_off, content_len = bl0 + 13, bl1 - bl0 - 13
    pre = (ctypes.c_void_p * 1)(base + bl0)
    pre_len = (ctypes.c_uint64 * 1)(13)
    blen = (ctypes.c_uint64 * 1)(content_len)
    bcrc = (ctypes.c_uint32 * 1)()
    rec = (ctypes.c_uint32 * 1)()

    def verify():
        got = [L.ambrycrc_update(0, base + a, b - a) for a, b in ranges[:-1]]
        bcrc[0] = L.ambrycrc_update(0, base + content_off, content_len)
        L.ambrycrc_put_crcs(None, None, pre, pre_len, bcrc, blen, 1, None, rec)
        return got + [rec[0]]

    vst, vend = ctypes.c_uint32(1), ctypes.c_uint64(0)

    def read():
        L.ambrycrc_verify_message_cpu(base, len(msg), 0, ctypes.byref(vst), ctypes.byref(vend))

    read()
    ok_r = vst.value == 0 and vend.value == len(msg)
    orc = Oracle()

    def oracle():
        return [orc.crc32(arr[a:b]) for a, b in ranges]

    ok_v, ok_o = verify() == expect, oracle() == expect
    reps = 20000
    res = {}
    for name, fn in (("write", write), ("verify", verify), ("read", read), ("oracle", oracle)):
        fn()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        res[name] = (time.perf_counter() - t0) / reps * 1e6
    crc_bytes = sum(b - a for a, b in ranges)
    result = {
        "metric": "us per 64 KiB PUT message through messageformat on the CPU (C1)",
        "value": round(res["write"], 3), "unit": "us", "n_gpus": 0, "steps": reps, "warmup": 1,
        "ms_per_step": round(res["write"] / 1e3, 6), "higher_is_better": False, "scaling": "none",
        "vs_baseline": None, "dtype": "u8", "data": "synthetic (splitmix64 bytes; the committed C1 fixture)",
        "config": {"workload": "C1: single 64 KiB blob PUT through messageformat on CPU",
                   "message_bytes": len(msg), "crc_bytes": crc_bytes, "records": fx["records"]},
        "product_write": {"us_per_message": round(res["write"], 3), "matches_fixture": ok_w,
                          "impl": L.ambrycrc_host_impl().decode(),
                          "what": "ambrycrc_serialize_put_host: header, key, records laid out, 4 CRC trailers, one core"},
        "product_verify": {"us_per_message": round(res["verify"], 3), "matches_fixture": ok_v,
                           "GiBps": round(crc_bytes / res["verify"] * 1e6 / 2**30, 2),
                           "what": "ambrycrc_update per record + ambrycrc_put_crcs for the blob record, one core"},
        "product_read": {"us_per_message": round(res["read"], 3), "clean": ok_r,
                         "what": "ambrycrc_verify_message_cpu: header, record versions and sizes, every CRC, one call"},
        "cpu_baseline": {"value": round(res["oracle"], 3), "unit": "us per message", "cores": 1, "kind": "port",
                         "matches_fixture": ok_o,
                         "sample": "the C1 message's four record CRCs, 20,000 repetitions; oracle/crc32_ref.c "
                                   "slice-by-8 restating Crc32.java:55-98"},
        "note": "every leg pays ~0.3 us of Python->C call overhead per call (write: 1; verify: 5; read: 1; oracle: 4)",
    }
    os.write(result_fd, (json.dumps(result) + "\n").encode())


# ------------------------------------------------------------------ main

def main():
    args = parse()
    # stdout carries exactly one JSON line (rank 0). Native libraries print to fd 1 on their
    # own (RCCL's version banner at communicator init), so fd 1 is pointed at stderr for
    # the run and the result is written to a saved copy of the original stdout.
    sys.stdout.flush()
    result_fd = os.dup(1)
    os.dup2(2, 1)
    if args.config == "c1":
        return run_c1(args, result_fd)
    import numpy as np
    import torch

    env_world = os.environ.get("WORLD_SIZE")
    if env_world is not None or args.force_dist:
        mode = "procs"  # one process per GPU (torchrun)
        world = int(env_world or "1")
        rank = int(os.environ.get("RANK", "0"))
        local = int(os.environ.get("LOCAL_RANK", "0"))
        if world != args.gpus:
            log(args, f"note: --gpus {args.gpus} but WORLD_SIZE={world}; using WORLD_SIZE")
        devices = [local]
    elif args.gpus > 1 or args.inproc:
        mode = "inproc"  # this process drives every GPU
        world, rank = args.gpus, 0
        if torch.cuda.device_count() < world:
            raise SystemExit(f"--gpus {world} but only {torch.cuda.device_count()} devices visible")
        devices = list(range(world))
    else:
        mode, world, rank, devices = "single", 1, 0, [0]
    config = args.config or ("c3" if world == 1 else "c5")
    if config == "c4" and mode != "single":
        raise SystemExit("c4 (verify-on-read) is a one-GPU config")

    from ambry_amd import device as D

    dist = None
    if mode == "procs":
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        # gloo is only the control plane (unique id, barriers, max of the timings); the data path's
        # collective is the RCCL all-gather inside libambrycrc
        dist.init_process_group("gloo")
    torch.cuda.set_device(devices[0])
    for d in devices:
        D.init(d)
        if args.variant is not None:
            D.set_variant(d, args.variant)
        if args.grid is not None:
            D.set_grid(d, args.grid)
        if args.window is not None:
            D.set_window(d, args.window)

    work = []
    for i, d in enumerate(devices):
        dev = torch.device("cuda", d)
        log(args, f"rank {rank + i}/{world} (device {d}): building workload {config}")
        with torch.cuda.device(dev):
            buf, off_t, len_t, n, total, chunk, desc = build_workload(torch, dev, config, rank + i)
            w = {"dev": dev, "buf": buf, "off": off_t, "len": len_t, "n": n, "total": total,
                 "stream": torch.cuda.current_stream(dev)}
            if mode != "single":
                w["gathered"] = torch.empty(world * n, dtype=torch.int32, device=dev)
        work.append(w)
    n, total = work[0]["n"], work[0]["total"]

    comm = None
    if mode == "procs":
        uid = [D.unique_id() if rank == 0 else None]
        dist.broadcast_object_list(uid, src=0)
        comm = D.Comm.rank(uid[0], world, rank, devices[0])
    elif mode == "inproc":
        comm = D.Comm.all_devices(devices)
    counts = [n] * world

    verify = None
    if config == "c4":
        # C4 is the verify-on-read path: expected CRCs from a clean pass, then single-bit flips
        # in 1 % of the chunks (seeded); each step recomputes and compares (ambrycrc_verify_dev).
        w = work[0]
        expected = D.crc32_batch(w["buf"], w["off"], w["len"]).clone()
        rng = np.random.default_rng(20261016 + rank)
        bad = np.sort(rng.choice(n, size=n // 100, replace=False))
        lens_h = w["len"].cpu().numpy()
        offs_h = w["off"].cpu().numpy()
        pos = offs_h[bad] + (rng.random(len(bad)) * lens_h[bad]).astype(np.int64)
        bits = torch.tensor(1 << rng.integers(0, 8, size=len(bad)), dtype=torch.uint8, device=w["dev"])
        pos_t = torch.tensor(pos, dtype=torch.int64, device=w["dev"])
        w["buf"][pos_t] ^= bits
        torch.cuda.synchronize()
        verify = {"expected": expected, "bad": bad, "out": torch.empty(n, dtype=torch.int32, device=w["dev"]),
                  "mism": torch.empty(n, dtype=torch.uint8, device=w["dev"])}

    def step():
        if mode == "single":
            w = work[0]
            if verify is not None:
                D.crc32_verify(w["buf"], w["off"], w["len"], verify["expected"], out=verify["out"],
                               mismatch=verify["mism"], count=False)
            else:
                w["out"] = D.crc32_batch(w["buf"], w["off"], w["len"])
        elif mode == "inproc":
            D.crc32_batch_multi_dev(comm, [dict(base=w["buf"], off=w["off"], len=w["len"], gathered=w["gathered"],
                                                stream=w["stream"]) for w in work])
        else:
            w = work[0]
            D.crc32_batch_gather(comm, w["buf"], w["off"], w["len"], w["gathered"], counts, stream=w["stream"])

    def sync_all():
        for w in work:
            torch.cuda.synchronize(w["dev"])

    # Clock ramp: the MI355X takes tens of ms of sustained load to reach its steady clocks
    # (a 0.7 ms C2 step measured 13 % slower over the first 20 steps than over 100). Run the
    # step untimed for >= --prewarm-s before the contract's W warmup steps.
    t_pre = time.perf_counter()
    while True:
        step()
        sync_all()
        if time.perf_counter() - t_pre >= args.prewarm_s:
            break
    for _ in range(args.warmup):
        step()
    sync_all()
    for w in work:
        D.timing_collect(w["dev"].index)  # drop warmup events
        D.timing_enable(w["dev"].index, True)
    if dist:
        dist.barrier()
    sync_all()
    t0 = time.perf_counter()
    ev0 = torch.cuda.Event(enable_timing=True)
    ev1 = torch.cuda.Event(enable_timing=True)
    ev0.record(work[0]["stream"])
    for _ in range(args.steps):
        step()
    ev1.record(work[0]["stream"])
    sync_all()
    if dist:
        dist.barrier()
    wall = time.perf_counter() - t0
    kern_each = []
    for w in work:
        D.timing_enable(w["dev"].index, False)
        kern_each += D.timing_collect_each(w["dev"].index)
    kern_ms, launches = sum(kern_each), len(kern_each)
    kern_median_ms = float(sorted(kern_each)[len(kern_each) // 2]) if kern_each else None
    ev_ms = ev0.elapsed_time(ev1)
    if args.dump_outputs and rank == 0:
        w = work[0]
        if mode != "single":
            outs = {"gathered_crc32": w["gathered"]}
        elif verify is not None:
            outs = {"crc32": verify["out"], "mismatch": verify["mism"]}
        else:
            outs = {"crc32": w["out"]}
        dump_outputs(args.dump_outputs, outs)

    elapsed = wall
    if dist:
        t = torch.tensor([wall], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    rccl = None
    if mode != "single" and args.full:
        # every GPU's gathered vector: its own slot equals its CRCs computed alone (untimed), and in
        # one process all GPUs hold the same vector
        ok = True
        for i, w in enumerate(work):
            with torch.cuda.device(w["dev"]):
                mine = D.crc32_batch(w["buf"], w["off"], w["len"])
                r = rank + i
                ok = ok and bool(torch.equal(w["gathered"][r * n:(r + 1) * n], mine))
        if mode == "inproc":
            g0 = work[0]["gathered"].cpu()
            ok = ok and all(torch.equal(g0, w["gathered"].cpu()) for w in work[1:])
        if dist:
            flag = torch.tensor([1 if ok else 0], dtype=torch.int32)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            ok = bool(flag.item())
        rccl = {"ranks": comm.size(), "allgather_ok": ok,
                "form": ("one process per GPU: ambrycrc_unique_id + ambrycrc_comm_init_rank, "
                         "ambrycrc_batch_dev_gather" if mode == "procs" else
                         "one process, N GPUs: ambrycrc_comm_init_all, ambrycrc_batch_dev_multi"),
                "gathered_crcs_per_gpu": world * n}
    w0 = work[0]
    with torch.cuda.device(w0["dev"]):
        read_roof = measure_read_roof(torch, D, w0["buf"], w0["buf"].numel(), w0["dev"].index) \
            if config != "c4" and args.full else None
    verify_ok = None
    if verify is not None and args.full:  # the flags must name exactly the flipped chunks
        flagged = np.nonzero(verify["mism"].cpu().numpy())[0]
        _, _, cnt = D.crc32_verify(w0["buf"], w0["off"], w0["len"], verify["expected"])  # counter form, untimed
        verify_ok = bool(np.array_equal(flagged, verify["bad"]) and int(cnt.item()) == len(verify["bad"]))
    value = world * total * args.steps / elapsed / 2**30
    kern_avg_s = kern_ms / max(1, launches) / 1e3
    alg_bytes = total + 4 * n  # chunk bytes read + 4 B CRC written per chunk (offset/len arrays excluded)
    achieved = alg_bytes / kern_avg_s / 1e9 if kern_avg_s > 0 else None
    traffic, traffic_src = traffic_for(config)

    if mode == "single":
        parallelism = "shard1"
    elif mode == "procs":
        parallelism = f"shard{world}+rccl_allgather (one process per GPU)"
    else:
        parallelism = f"shard{world}+rccl_allgather (one process, {world} GPUs)"
    result = {
        "metric": METRIC,
        "value": round(value, 2),
        "unit": "GiB/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(elapsed / args.steps * 1e3, 4),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "u8",
        "data": "synthetic (device splitmix64 bytes; no dataset)",
        "config": {"workload": desc, "chunks_per_gpu": n, "chunk_bytes": CONFIGS.get(config, (0, None))[1],
                   "bytes_per_gpu_step": total, "parallelism": parallelism,
                   "kernel_variant": D.get_variant(w0["dev"].index),
                   "grid_workgroups": D.grid_size(w0["dev"].index),
                   "sweep_window_bytes": args.window if args.window is not None else 32 << 30},
        "roofline": {
            "bound": "hbm",
            "kernel": "crc32_sweep_kernel",
            "achieved": round(achieved, 1) if achieved else None,
            "peak": HBM_PEAK_GBS,
            "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBS, 4) if achieved else None,
            "traffic": traffic,
            "traffic_source": traffic_src,
            "traffic_over_algorithmic": round(traffic / alg_bytes, 5) if traffic else None,
            "kernel_avg_ms": round(kern_avg_s * 1e3, 4),
            "kernel_median_ms": round(kern_median_ms, 4) if kern_median_ms else None,
            "algorithmic_bytes_per_launch": alg_bytes,
            "value_frac_of_peak": round(value * 2**30 / 1e9 / world / HBM_PEAK_GBS, 4),
            "measured_read_roof": read_roof,
            "frac_of_measured_read_roof": (round(achieved / read_roof, 4)
                                           if achieved and read_roof else None),
        },
        "timing": {"wall_s": round(elapsed, 4), "stream_event_ms": round(ev_ms, 3), "kernel_launches": launches},
        "allgather_ok": None if rccl is None else rccl["allgather_ok"],
        "rccl": rccl,
        "verify": (None if verify is None else
                   {"flipped_chunks": int(len(verify["bad"])), "flags_exact": verify_ok,
                    "what": "ambrycrc_verify_dev per step: CRCs recomputed and compared with the clean pass; "
                            "single-bit flips in 1 % of chunks (seeded)"}),
    }

    if args.full and rank == 0 and world == 1:
        if not args.no_cpu_baseline:
            log(args, "cpu baseline")
            cb = cpu_baseline(w0["buf"], w0["off"], w0["len"], n, args)
            if cb is not None:
                ref = cb.pop("_out")
                if mode == "single":
                    crcs = (w0["out"] if verify is None else verify["out"]).cpu().numpy().view("uint32")
                else:
                    crcs = w0["gathered"][:n].cpu().numpy().view("uint32")
                cb["parity_vs_gpu"] = bool((ref == crcs[:len(ref)]).all())
                result["cpu_baseline"] = cb
        if not args.no_host_path and config == "c3":
            log(args, "host-resident path")
            for w in work:
                del w["buf"]
            torch.cuda.empty_cache()
            result["host_path"] = host_path_rate(torch, args)
    if rank == 0:
        sys.stdout.flush()
        os.write(result_fd, (json.dumps(result) + "\n").encode())
    if comm is not None:
        comm.destroy()
    if dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
