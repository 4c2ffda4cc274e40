"""The argument checks of every device wrapper of ambry_amd.device and ambry_amd.messages, as a table: a valid call
on m = 2 stored PUTs of about 200 B (the smallest batch that tells "m elements" from "1 element"), then for each
tensor argument each mutation its check covers -- a wrong dtype, a CPU tensor, a numel off by one, a
non-contiguous view -- which must raise TypeError before anything is launched.

Rows marked T are the tightenings of DESIGN.md §21: checks the wrapper did not make before the shared argument
layer. With AMBRYCRC_ARGS_BASELINE=1 in the environment the file describes the code before that layer: a T row
must then not raise, and a T row whose misread argument could make a kernel write out of bounds (T_UNSAFE) is
not run at all."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import ingest_oracle as IO
import rekey_oracle as RK
from datagen import stream_bytes
from msgfmt import MF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASELINE = os.environ.get("AMBRYCRC_ARGS_BASELINE") == "1"
M_MSGS = 2
T, T_UNSAFE = "T", "T_UNSAFE"


# ---------------------------------------------------------------- the valid calls
def _stored_puts(m):
    msgs = [RK.stored_put(MF.store_key("w%d" % k), MF.blob_properties_bytes(100 + k), b"u" * 5,
                          stream_bytes(70 + k, 0, 100 + k).tobytes()) for k in range(m)]
    offs = np.cumsum([0] + [len(x) for x in msgs[:-1]]).astype(np.int64)
    return b"".join(msgs), offs, np.array([len(x) for x in msgs], dtype=np.int64)


def _frames(m):
    keys = [MF.store_key("f%d" % k) for k in range(m)]
    frames = [IO.frame(5, keys[k], MF.blob_properties_bytes(90 + k), b"um", stream_bytes(80 + k, 0, 90 + k).tobytes())
              for k in range(m)]
    refs = np.zeros(m, dtype=IO.REF)
    refs["off"] = np.cumsum([0] + [len(f) for f in frames[:-1]])
    refs["key_len"] = [len(k) for k in keys]
    return b"".join(frames), refs


def build_calls(m):
    """{wrapper name: (function of the tensor arguments by name, the valid tensor arguments)} on m messages."""
    import torch

    from ambry_amd import device as D
    from ambry_amd import messages as M

    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    i64 = lambda a: torch.tensor(np.asarray(a, dtype=np.int64), device="cuda")  # noqa: E731
    u8 = lambda n: torch.zeros(n, dtype=torch.uint8, device="cuda")  # noqa: E731
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device="cuda")  # noqa: E731
    region_b, offs, sizes = _stored_puts(m)
    region, n = dev(np.frombuffer(region_b, dtype=np.uint8)), len(region_b)
    wire_b, refs = _frames(m)
    trailed = np.frombuffer(b"".join(x + MF._crc_long(x) for x in [b"abc" * 9] * m), dtype=np.uint8)
    packed = M.pack_batch([M.PutMessage(key=b"k" * 24, props=MF.blob_properties_bytes(50), usermeta=b"um",
                                        blob=b"b" * (50 + k)) for k in range(m)])
    rk = np.zeros(m, dtype=M.REKEY_DESC_DTYPE)
    rk["key_src"], rk["key_len"], rk["content_src"], rk["props_blob_size"] = np.arange(m) * 30, 30, M.REKEY_KEEP, -1
    st, plan = D.hard_delete_messages(region.clone(), i64(offs), plan_only=True)
    torch.cuda.synchronize()
    assert int(st.abs().sum().item()) == 0
    batch = dict(base=region, off=i64(offs), len=i64(sizes))
    return {
        "crc32_batch": (lambda a: D.crc32_batch(a["base"], a["off"], a["len"], a["crc_in"], a["out"], a["workspace"]),
                        dict(batch, crc_in=i32(m), out=i32(m), workspace=u8(D.workspace_bytes(m)))),
        "crc32_verify": (lambda a: D.crc32_verify(a["base"], a["off"], a["len"], a["expected"], a["crc_in"],
                                                  a["out"], mismatch=a["mismatch"]),
                         dict(batch, expected=i32(m), crc_in=i32(m), out=i32(m), mismatch=u8(m))),
        "verify_trailed": (lambda a: D.verify_trailed(a["base"], a["off"], a["len"]),
                           dict(base=dev(trailed), off=i64(np.arange(m) * 35), len=i64([35] * m))),
        "verify_messages": (lambda a: D.verify_messages(a["region"], a["msg_off"]),
                            dict(region=region, msg_off=i64(offs))),
        "hard_delete_messages": (lambda a: D.hard_delete_messages(a["region"], a["msg_off"], a["recovery"],
                                                                  workspace=a["workspace"]),
                                 dict(region=region.clone(), msg_off=i64(offs), recovery=plan.reshape(-1),
                                      workspace=u8(D.hard_delete_workspace_bytes(m)))),
        "chain_messages": (lambda a: D.chain_messages(a["region"], 0, m, workspace=a["workspace"]),
                           dict(region=region, workspace=u8(D.chain_workspace_bytes(n, m)))),
        "recover_messages": (lambda a: D.recover_messages(a["region"], 0, m, workspace=a["workspace"]),
                             dict(region=region, workspace=u8(D.recover_workspace_bytes(n, m)))),
        "serialize_dev": (lambda a: M.serialize_dev(a["descs"], a["out"], a["fields"], a["blobs"], a["msg_len"]),
                          dict(descs=dev(packed[0]), out=u8(packed[4]), fields=dev(np.frombuffer(packed[1], np.uint8)),
                               blobs=dev(np.frombuffer(packed[2], np.uint8)), msg_len=i64([0] * m))),
        "transform_dev": (lambda a: M.transform_dev(a["region"], a["msg_off"], life_version=a["life_version"],
                                                    out=a["out"]),
                          dict(region=region, msg_off=i64(offs), out=u8(M.out_bound(n, m)),
                               life_version=torch.zeros(m, dtype=torch.int16, device="cuda"))),
        "rekey_dev": (lambda a: M.rekey_dev(a["region"], a["msg_off"], a["descs"], a["aux"],
                                            life_version=a["life_version"], out=a["out"], workspace=a["workspace"]),
                      dict(region=region, msg_off=i64(offs), descs=dev(rk), aux=u8(30 * m) + 7,
                           life_version=torch.zeros(m, dtype=torch.int16, device="cuda"),
                           out=u8(M.rekey_out_bound(n, m, 30 * m)), workspace=u8(M.rekey_workspace_bytes(m)))),
        "ingest_put_requests_dev": (lambda a: M.ingest_put_requests_dev(a["wire"], a["refs"], out=a["out"],
                                                                        workspace=a["workspace"]),
                                    dict(wire=dev(np.frombuffer(wire_b, np.uint8)), refs=dev(refs),
                                         out=u8(M.ingest_out_bound(len(wire_b), m)),
                                         workspace=u8(M.ingest_workspace_size(m)))),
        "send_messages_dev": (lambda a: M.send_messages_dev(a["region"], a["msg_off"], M.SEND_ALL, a["msg_size"],
                                                            out=a["out"], workspace=a["workspace"]),
                              dict(region=region, msg_off=i64(offs), msg_size=i64(sizes), out=u8(n),
                                   workspace=u8(M.send_workspace_bytes(m)))),
        "receive_blobs_dev": (lambda a: M.receive_blobs_dev(a["body"], a["pay_off"], M.SEND_ALL, a["pay_size"],
                                                            a["ranges"], a["dst_off"], out=a["out"],
                                                            workspace=a["workspace"]),
                              dict(body=region, pay_off=i64(offs), pay_size=i64(sizes), ranges=i64([0, -1] * m),
                                   dst_off=i64(np.arange(m) * 128), out=u8(n),
                                   workspace=u8(M.receive_workspace_bytes(m)))),
    }


@pytest.fixture(scope="module")
def wrappers(gpu):
    return build_calls(M_MSGS)


# ---------------------------------------------------------------- the table
# wrapper -> argument -> {mutation: "" (checked before and after) | T | T_UNSAFE}; an absent mutation is one the
# argument's check does not cover (any capacity goes for an output buffer, any dtype for a workspace, and the
# argument that defines the batch size has no numel to be off)
ALL = ("dtype", "cpu", "numel", "strided")


def _row(muts=ALL, **flags):
    return {k: flags.get(k, "") for k in muts}


DATA = _row(("dtype", "cpu", "strided"))              # a byte buffer of any size
DATA_T = _row(("dtype", "cpu", "strided"), strided=T)  # ... whose contiguity was not checked
WS = _row(("cpu", "strided"))
BATCH = {"base": DATA_T, "off": DATA, "len": _row()}
TABLE = {
    "crc32_batch": dict(BATCH, crc_in=_row(), out=_row(), workspace=WS),
    "crc32_verify": dict(BATCH, expected=_row(), crc_in=_row(), out=_row(), mismatch=_row()),
    "verify_trailed": BATCH,
    "verify_messages": {"region": DATA_T, "msg_off": DATA},
    "hard_delete_messages": {"region": DATA, "msg_off": DATA, "recovery": _row(), "workspace": WS},
    # (the tensors of `out` are the caller's own from an earlier call: not checked)
    "chain_messages": {"region": DATA, "workspace": WS},
    "recover_messages": {"region": DATA, "workspace": WS},
    # descs read as dense from a strided view are garbage offsets for the writer: not run on the old code
    "serialize_dev": {"descs": _row(strided=T_UNSAFE), "out": DATA_T, "fields": DATA_T, "blobs": DATA_T,
                      "msg_len": _row(strided=T)},
    "transform_dev": {"region": DATA_T, "msg_off": DATA, "life_version": _row(), "out": DATA},
    "rekey_dev": {"region": DATA_T, "msg_off": DATA, "descs": _row(), "aux": DATA, "life_version": _row(),
                  "out": DATA, "workspace": WS},
    "ingest_put_requests_dev": {"wire": DATA, "refs": _row(), "out": DATA, "workspace": WS},
    "send_messages_dev": {"region": DATA_T, "msg_off": DATA, "msg_size": _row(), "out": DATA, "workspace": WS},
    "receive_blobs_dev": {"body": DATA_T, "pay_off": DATA, "pay_size": _row(), "ranges": _row(), "dst_off": _row(),
                          "out": DATA, "workspace": WS},
}
ROWS = [(w, a, mut, flag) for w, args in TABLE.items() for a, muts in args.items() for mut, flag in muts.items()]


def mutate(t, mut):
    import torch

    if mut == "dtype":  # another dtype of the same width: the bytes and the byte size stay
        return t.view({1: torch.int8, 2: torch.float16, 4: torch.float32, 8: torch.float64}[t.element_size()])
    if mut == "cpu":
        return t.cpu()
    if mut == "numel":
        return torch.cat([t, t[:1]])
    return t.repeat_interleave(2)[::2]  # the same values, every other element of a doubled tensor


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TABLE))
def test_valid_call(wrappers, name):
    import torch

    call, args = wrappers[name]
    assert set(args) == set(TABLE[name])
    call(args)
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("name,arg,mut,flag", ROWS, ids=["%s-%s-%s" % r[:3] for r in ROWS])
def test_mutation_raises_type_error(wrappers, name, arg, mut, flag):
    import torch

    call, args = wrappers[name]
    bad = mutate(args[arg], mut)
    assert bad.numel() == args[arg].numel() + (mut == "numel") and (mut != "strided" or not bad.is_contiguous())
    if BASELINE and flag == T_UNSAFE:
        return
    if BASELINE and flag == T:
        call(dict(args, **{arg: bad}))
        torch.cuda.synchronize()
        return
    with pytest.raises(TypeError, match=arg):
        call(dict(args, **{arg: bad}))


# ---------------------------------------------------------------- without a GPU
def test_cpu_tensor_as_first_argument():
    """The first argument of every device wrapper is refused when it lives on the host, before torch.cuda or the
    library is touched."""
    import torch

    from ambry_amd import device as D
    from ambry_amd import messages as M

    r = torch.zeros(256, dtype=torch.uint8)
    o = torch.zeros(2, dtype=torch.int64)
    for call in (lambda: D.crc32_batch(r, o, o), lambda: D.crc32_verify(r, o, o, o.to(torch.int32)),
                 lambda: D.verify_trailed(r, o, o), lambda: D.verify_messages(r, o),
                 lambda: D.hard_delete_messages(r, o), lambda: D.chain_messages(r), lambda: D.recover_messages(r),
                 lambda: D.fill_random(r, 1), lambda: M.serialize_dev(r[:160], r), lambda: M.transform_dev(r, o),
                 lambda: M.rekey_dev(r, o, r[:80], r), lambda: M.ingest_put_requests_dev(r, r[:32]),
                 lambda: M.send_messages_dev(r, o, M.SEND_ALL), lambda: M.receive_blobs_dev(r, o, M.SEND_ALL)):
        with pytest.raises(TypeError):
            call()


@pytest.mark.skipif(BASELINE, reason="the host-buffer coercer is part of the argument layer")
def test_host_buffer_coercer():
    import torch

    from ambry_amd._args import host_buffer

    data = bytes(range(40))
    for buf in (data, bytearray(data), memoryview(data), np.frombuffer(data, dtype=np.uint8),
                torch.frombuffer(bytearray(data), dtype=torch.uint8)):
        keep, addr, n = host_buffer("region", buf)
        assert n == 40 and ctypes.string_at(addr, n) == data
        del keep
    for empty in (b"", bytearray(), np.zeros(0, dtype=np.uint8)):
        assert host_buffer("region", empty)[1:] == (0, 0)
    ba = bytearray(data)
    keep, addr, n = host_buffer("region", ba, writable=True)
    assert n == 40 and addr
    ro = np.frombuffer(data, dtype=np.uint8)
    assert not ro.flags.writeable
    for refused in (data, ro, memoryview(data)):
        with pytest.raises(TypeError, match="region"):
            host_buffer("region", refused, writable=True)
    for refused in (np.zeros(4, dtype=np.int32), 7, None):
        with pytest.raises(TypeError, match="region"):
            host_buffer("region", refused)
    strided = np.arange(8, dtype=np.uint8)[::2]  # read through a contiguous copy, never written through one
    keep, addr, n = host_buffer("region", strided)
    assert ctypes.string_at(addr, n) == bytes([0, 2, 4, 6])
    with pytest.raises(TypeError, match="region"):
        host_buffer("region", strided, writable=True)


def test_import_without_torch():
    code = ("import sys; import ambry_amd, ambry_amd.device, ambry_amd.messages; "
            "assert 'torch' not in sys.modules, 'torch imported'")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT, capture_output=True, timeout=60)
