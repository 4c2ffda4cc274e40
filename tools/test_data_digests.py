#!/usr/bin/env python3
"""One SHA-256 per test-data case: every region / message builder and every oracle expected() that the test
support modules hold, called with the arguments the suite uses, printed as one JSON object. A change that moves
or merges test support runs this before and after on the same machine and compares the two outputs; the
comparison of record is profiles/test_support_refactor.json. Not a test: numpy's generator streams are not
guaranteed stable across numpy versions, so the digests hold for one machine only."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

# ---- imports: the one part that differs between the two runs
import hard_delete_oracle as HD  # noqa: E402
import ingest_oracle as IO  # noqa: E402
import recover_oracle as RO  # noqa: E402
import recv_oracle as RV  # noqa: E402
import rekey_oracle as RK  # noqa: E402
import scale_tiles as S  # noqa: E402
import send_oracle as SO  # noqa: E402
from msgfmt import MF  # noqa: E402
from oracle_common import add_seconds_to_epoch  # noqa: E402
from regions import (dense_old_region, dense_v3_region, join, make_requests, put_expected,  # noqa: E402
                     random_messages, record_level_cases, refused_messages, replica_region, verify_region)

rekey_region, stored_put, metadata_region = RK.build_region, RK.stored_put, RK.metadata_region
recover_put, recover_update, sized_put = RO.put_message, RO.update_message, RO.sized_put
# ---- end of imports


def feed(h, x):
    """x into the hash, with its type and length so that neighbouring values cannot run together."""
    if x is None or isinstance(x, (bool, int, float, str, np.integer, np.floating, np.bool_)):
        h.update(("%s:%r;" % (type(x).__name__.rstrip("_0123456789"), x if x is None else x.item()
                              if isinstance(x, np.generic) else x)).encode())
    elif isinstance(x, (bytes, bytearray)):
        h.update(b"b%d:" % len(x) + bytes(x))
    elif isinstance(x, np.ndarray):
        h.update(("a%s%s:" % (x.dtype.descr, x.shape)).encode() + np.ascontiguousarray(x).tobytes())
    elif isinstance(x, np.void):
        feed(h, np.asarray(x))
    elif isinstance(x, (list, tuple)):
        h.update(b"l%d:" % len(x))
        for y in x:
            feed(h, y)
    elif isinstance(x, dict):
        h.update(b"d%d:" % len(x))
        for k in sorted(x):
            feed(h, k)
            feed(h, x[k])
    elif hasattr(x, "__dict__"):
        feed(h, {k: v for k, v in vars(x).items() if not k.startswith("_")})
    else:
        raise TypeError("no digest for %r" % type(x))


def digest(x) -> str:
    h = hashlib.sha256()
    feed(h, x)
    return h.hexdigest()


def tight(lengths) -> int:
    """An out_cap that refuses about half of a batch for room."""
    return int(sum(int(n) for n in lengths)) // 2 + 1


def cases():
    out = {}

    def add(name, value):
        assert name not in out, name
        out[name] = digest(value)

    # -- the verify region (status per message) and the replica region of the transform tests
    add("verify_region()", verify_region())
    for kw in (dict(n=120, corrupt_frac=0.0), dict(n=300, seed=1, corrupt_frac=0.1, big_every=17),
               dict(n=500, seed=31, corrupt_frac=0.1), dict(n=700, seed=40, corrupt_frac=0.08, big_every=10**9),
               dict(n=300, seed=4, corrupt_frac=0.0, big_every=50), dict(n=40, seed=5, corrupt_frac=0.2, big_every=10**9)):
        add("verify_region(%s)" % kw, verify_region(**kw))
    for m in (1, 1024, 1025):  # test_gpu_hard_delete.exact_case
        region, offs, _ = verify_region(n=m + 1, seed=700 + m, corrupt_frac=0.1 if m > 1 else 0.0, big_every=10**9)
        region, offs = region[offs[1]:], [o - offs[1] for o in offs[1:]]
        add("hard_delete exact_case(%d)" % m, (region, offs))
        add("hard_delete exact_case(%d) expected" % m, HD.hard_delete(region, offs))
    for n, seed, corrupt in ((600, 34, True), (600, 32, True), (300, 53, True), (40, 5, False), (120, 22, True)):
        add("replica_region(%d, seed=%d, corrupt=%s)" % (n, seed, corrupt), replica_region(n, seed=seed, corrupt=corrupt))
    for n, seed, kw in ((200, 61, {}), (400, 71, {}), (409, 1309, {}), (65, 67, dict(lead=2, trail=29))):
        add("dense_v3_region(%d, seed=%d, %s)" % (n, seed, kw), dense_v3_region(n, seed=seed, **kw))
    for n, seed in ((700, 5), (200, 5), (300, 9)):
        add("dense_old_region(%d, seed=%d)" % (n, seed), dense_old_region(n, seed=seed))
    add("record_level_cases()", record_level_cases())
    add("refused_messages(64, 'r64')", refused_messages(64, "r64"))
    add("make_requests()", make_requests())
    add("make_requests(n=12, seed=9)", make_requests(n=12, seed=9))

    # -- the write side
    for n, seed, kw in ((300, 11, {}), (400, 102, {}), (1, 601, dict(max_blob=600)), (300, 21, dict(max_blob=9000))):
        msgs = random_messages(n, seed, **kw)
        add("random_messages(%d, %d, %s)" % (n, seed, kw), msgs)
        add("put_expected of random_messages(%d, %d, %s)" % (n, seed, kw), [put_expected(m) for m in msgs])

    # -- re-key: the region of every stored format, its descriptors, the oracle with and without room
    for seed in (1, 2, 3):
        region, offs, meta = rekey_region(n=300, seed=seed)
        descs, aux = RK.build_descs(offs, meta, seed=seed)
        add("rekey_region(n=300, seed=%d)" % seed, (region, offs, meta))
        add("rekey build_descs(seed=%d)" % seed, (descs, aux))
        full = RK.expected(region, offs, descs, aux)
        add("rekey expected(seed=%d)" % seed, full)
        add("rekey expected(seed=%d, tight out_cap)" % seed,
            RK.expected(region, offs, descs, aux, out_cap=tight(full[2])))
    for m in (1, 512, 513):  # test_gpu_rekey.exact_case
        region, offs, meta = rekey_region(n=m, seed=800 + m, corrupt_frac=0.1 if m > 1 else 0.0, big_every=10**9,
                                          max_blob=600, max_usermeta=300)
        descs, aux = RK.build_descs(offs, meta, seed=800 + m)
        add("rekey exact_case(%d)" % m, (region, offs, descs, aux, RK.expected(region, offs, descs, aux)))
    meta_case = metadata_region([0, 1, 63, 64, 65, 4096, 70000])
    add("metadata_region", meta_case)
    add("metadata_region expected v1", RK.expected(*meta_case, version=1))
    add("stored_put", stored_put(MF.store_key("b7"), MF.blob_properties_bytes(7, serde_version=3), b"u" * 7, b"c" * 7,
                                 hv=2, bv=2, enc_key=b"e" * 9))

    # -- send and receive
    for m, flag in ((1, SO.ALL), (2048, SO.ALL), (2049, SO.BLOB)):  # test_gpu_send.exact_case
        region, offs, _ = rekey_region(n=m, seed=1000 + m, corrupt_frac=0.1 if m > 1 else 0.0, big_every=10**9,
                                       max_blob=600, max_usermeta=300)
        ends = offs[1:] + [len(region)]
        sizes = [SO.header_length(region, o) or e - o for o, e in zip(offs, ends)] if flag == SO.ALL else None
        add("send exact_case(%d, %d)" % (m, flag), (region, offs, sizes, SO.expected(region, offs, sizes, flag)))
    names, region, offs, sizes = SO.rule_cases()
    add("send rule_cases()", (names, region, offs, sizes))
    for flag in SO.FLAGS:
        for sz in (None, sizes):
            full = SO.expected(region, offs, sz, flag)
            add("send expected(rule_cases, flag=%d, sized=%s)" % (flag, sz is not None), full)
            add("send expected(rule_cases, flag=%d, sized=%s, tight out_cap)" % (flag, sz is not None),
                SO.expected(region, offs, sz, flag, out_cap=tight(full[1]["send_len"])))
    region, offs, _ = rekey_region(n=300, seed=1)
    for flag in SO.FLAGS:
        full = SO.expected(region, offs, None, flag)
        add("send expected(region 1, flag=%d)" % flag, full)
        add("send expected(region 1, flag=%d, tight out_cap)" % flag,
            SO.expected(region, offs, None, flag, out_cap=tight(full[1]["send_len"])))
    add("recv rule_cases()", RV.rule_cases())
    for name, payload, flag, lo, hi, cap, _want in RV.rule_cases():
        add("recv expected(rule %s)" % name, RV.expected(payload, [0], None, flag, [(lo, hi)], out_cap=cap))
    for flag in (RV.BLOB, RV.ALL):
        body, po, ps = RV.sent_region(flag)
        add("recv sent_region(%d)" % flag, (body, po, ps))
        full = RV.expected(body, po, ps, flag)
        add("recv expected(sent_region(%d))" % flag, full)
        add("recv expected(sent_region(%d), tight out_cap)" % flag,
            RV.expected(body, po, ps, flag, out_cap=tight(full[1]["out_len"])))
        ranges = RV.some_ranges(body, po, ps, flag)
        add("recv expected(sent_region(%d), ranges)" % flag, RV.expected(body, po, ps, flag, ranges))

    # -- recover
    add("recover stop_cases()", RO.stop_cases())
    add("recover mixed_region()", RO.mixed_region())
    add("recover residue_region()", RO.residue_region())
    for hv in (1, 2, 3):
        for partial in (False, True):
            region = RO.recovery_test_region(hv, partial)
            add("recover recovery_test_region(%d, %s)" % (hv, partial), region)
            add("recover recover(recovery_test_region(%d, %s))" % (hv, partial), RO.recover(region[0]))
    for name, region in RO.stop_cases():
        add("recover recover(stop %s)" % name, RO.recover(region))
    add("recover false_node_region()", RO.false_node_region())
    add("recover messages", (recover_put(MF.store_key("p"), b"content", hv=2, um=b"um", ttl=5),
                             recover_update(MF.store_key("u"), hv=1, uv=2), sized_put(MF.store_key("s"), 193, hv=1),
                             join([b"ab", b"cde", b""])))
    for a, b in ((-1, 5), (5, -1), (1_700_000_000_000, 9999), ((1 << 63) - 5, 1), (7, (1 << 62)), (7, -(1 << 62)),
                 (-(1 << 63), -1000)):
        add("add_seconds(%d, %d)" % (a, b), add_seconds_to_epoch(a, b))

    # -- ingest
    for args, kw in (((300, 1), {}), ((300, 2), {}), ((300, 3), {}),
                     ((409, 1209), dict(refused=0.1, blobs=(0, 1, 63, 300, 600))), ((1, 801), dict(refused=0.0, blobs=(0, 1, 63, 300, 600)))):
        wire, refs, kinds = IO.build_wire(*args, **kw)
        add("ingest build_wire(%s, %s)" % (args, kw), (wire, refs, kinds))
        for version in (3, 1):
            full = IO.expected(wire, refs, header_version=version)
            add("ingest expected(build_wire(%s), v%d)" % (args, version), full)
            add("ingest expected(build_wire(%s), v%d, tight out_cap)" % (args, version),
                IO.expected(wire, refs, header_version=version, out_cap=tight(full[3])))
    add("ingest tile_case()", IO.tile_case())

    # -- the scale tile and the oracles over it
    t = S.tile()
    add("scale tile()", t)
    add("scale verify_oracle", S.verify_oracle(t.region, t.offs))
    add("scale transform_oracle", S.transform_oracle(t.region, t.offs, t.life, 3))
    add("scale hard_delete_oracle", S.hard_delete_oracle(t.region, t.offs))
    full = S.rekey_oracle(t.region, t.offs, t.descs, t.aux)
    add("scale rekey_oracle", full)
    add("scale rekey_oracle(tight out_cap)", S.rekey_oracle(t.region, t.offs, t.descs, t.aux, out_cap=tight(full[2])))
    msgs = S.clean_puts(t.region, t.offs, S.verify_oracle(t.region, t.offs)[0])
    add("scale serialize_oracle", S.serialize_oracle(msgs))
    return out


if __name__ == "__main__":
    json.dump(cases(), sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write("\n")
