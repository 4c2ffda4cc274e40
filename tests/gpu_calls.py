"""The device calls that more than one GPU test module makes: each feature's entry run over guarded buffers
(gpu_buffers.py) with its outputs fetched to the host, the comparison of those outputs with the feature's oracle,
and the tiled buffers of the tests above the capped grids. torch and the library are imported inside the
functions."""
import numpy as np

import hard_delete_oracle as HD
import ingest_oracle as IO
import recover_oracle as RO
import scale_tiles as S
import send_oracle as SO
from gpu_buffers import guarded, guards_intact, u64_dev
from oracle_common import same


def unchanged(whole, shift: int, data: bytes, what: str):
    """The guards around an input hold and the input is as it was."""
    same(guards_intact(whole, shift, len(data)).tobytes(), data, "%s after the call" % what)


# ---------------------------------------------------------------- hard delete
def recovery_dev(info):
    """HD.INFO records as the (m, 32) uint8 tensor the hard delete takes for its recovery infos."""
    import torch

    return torch.from_numpy(np.ascontiguousarray(info).view(np.uint8).reshape(len(info), 32)).cuda()


def run_hard_delete(gpu, region: bytes, offs, shift=0, recovery=None, plan_only=False, workspace=None):
    import torch

    whole, r = guarded(region, shift)
    o = torch.tensor(np.asarray(offs, dtype=np.int64), device="cuda")
    status, info = gpu.hard_delete_messages(r, o, recovery=None if recovery is None else recovery_dev(recovery),
                                            plan_only=plan_only, workspace=workspace)
    torch.cuda.synchronize()
    return (status.cpu().numpy().view(np.uint32).tolist(), info.cpu().numpy().reshape(-1).view(HD.INFO),
            guards_intact(whole, shift, len(region)).tobytes())


# ---------------------------------------------------------------- re-key
def run_rekey(messages, region: bytes, offs, descs, aux: bytes, shift=0, oshift=0, life=None, version=3, out_cap=None,
              workspace=None):
    """(status, out_off, out_len lists, the output view's bytes): guards checked around the region (which must
    be unchanged), aux and the output."""
    import torch

    rw, r = guarded(region, shift)
    aw, a = guarded(aux, 5)
    cap = messages.rekey_out_bound(len(region), len(offs), len(aux)) if out_cap is None else out_cap
    ow, o = guarded(b"", oshift, cap)
    mo = u64_dev(offs)
    dd = torch.from_numpy(np.ascontiguousarray(descs).view(np.uint8).reshape(-1).copy()).cuda()
    lv = None if life is None else torch.tensor(np.asarray(life, dtype=np.int16), device="cuda")
    _, out_off, out_len, status = messages.rekey_dev(r, mo, dd, a, header_version=version, life_version=lv, out=o,
                                                     workspace=workspace)
    torch.cuda.synchronize()
    unchanged(rw, shift, region, "the region")
    unchanged(aw, 5, aux, "aux")
    return (status.cpu().numpy().view(np.uint32).tolist(), out_off.cpu().numpy().view(np.uint64).tolist(),
            out_len.cpu().numpy().view(np.uint64).tolist(), guards_intact(ow, oshift, cap))


def assert_rekey_outputs(got, exp):
    """Status, placement and every byte of every written span."""
    st, off, ln, out = got
    est, eoff, eln, packed = exp
    same(st, est, "status")
    same(off, eoff, "out_off")
    same(ln, eln, "out_len")
    for o, n in zip(eoff, eln):
        if n:
            assert out[o:o + n].tobytes() == packed[o:o + n], "message at output offset %d differs" % o


# ---------------------------------------------------------------- send
def run_send(messages, region: bytes, offs, sizes, flag, shift=0, oshift=0, out_cap=64, workspace=None):
    """(status list, INFO array, the output view's bytes): guards checked around the region (which must be
    unchanged) and the output."""
    import torch

    rw, r = guarded(region, shift)
    ow, o = guarded(b"", oshift, out_cap)
    mo = u64_dev(offs)
    ms = None if sizes is None else u64_dev(sizes)
    _, info, status = messages.send_messages_dev(r, mo, flag, msg_size=ms, out=o, workspace=workspace)
    torch.cuda.synchronize()
    unchanged(rw, shift, region, "the region")
    return (status.cpu().numpy().view(np.uint32).tolist(), info.cpu().numpy().view(SO.INFO),
            guards_intact(ow, oshift, out_cap))


def assert_send_outputs(got, exp):
    """Status, every info field, every byte of every sent span, and 0xA5 everywhere else."""
    st, info, out = got
    est, einfo, packed = exp
    same(st, list(est), "status")
    same(info, einfo, "info")
    untouched = np.ones(len(out), dtype=bool)
    for f in einfo:
        o, n = int(f["out_off"]), int(f["send_len"])
        if n:
            assert out[o:o + n].tobytes() == packed[o:o + n], "span at output offset %d differs" % o
            untouched[o:o + n] = False
    assert (out[untouched] == 0xA5).all(), "bytes written outside the sent spans"


def check_send(messages, region, offs, sizes, flag, shift=0, oshift=0, out_cap=None, cpu=False, slack=0,
               workspace=None, exp=None):
    """The batch on the device against the oracle (and the CPU entry), out_cap by default exactly the sum of the
    sent spans plus `slack`. Returns the oracle's answers."""
    exp = SO.expected(region, offs, sizes, flag, out_cap=out_cap) if exp is None else exp
    cap = max(len(exp[2]) + slack, 1) if out_cap is None else out_cap
    got = run_send(messages, region, offs, sizes, flag, shift, oshift, cap, workspace)
    assert_send_outputs(got, exp)
    if cpu:
        cst, cinfo, cout = SO.run_cpu(messages, region, offs, sizes, flag, out_cap=out_cap)
        same(cst, got[0], "status of the CPU entry against the device's")
        same(cout, exp[2], "output of the CPU entry against the oracle's")
        same(cinfo, got[1], "info of the CPU entry against the device's")
    return exp


# ---------------------------------------------------------------- recover
def recover_to_numpy(out):
    """A device call's tensors as the CPU entry's numpy arrays."""
    if len(out) == 2:
        return out[0].cpu().numpy().view(np.uint64), np.frombuffer(out[1].cpu().numpy().tobytes(), dtype=RO.RESULT)[0]
    msg_off, info, status, result = out
    return (msg_off.cpu().numpy().view(np.uint64), info.cpu().numpy().reshape(-1).view(RO.INFO),
            status.cpu().numpy().view(np.uint32), np.frombuffer(result.cpu().numpy().tobytes(), dtype=RO.RESULT)[0])


def run_recover(dev, region: bytes, start=0, max_m=64, shift=0, chain=False, workspace=None):
    import torch

    rw, r = guarded(region, shift)
    out = (dev.chain_messages if chain else dev.recover_messages)(r, start, max_m, workspace=workspace)
    torch.cuda.synchronize()
    unchanged(rw, shift, region, "the region")
    return recover_to_numpy(out)


def assert_chain(got, offs, res, max_m):
    """A chain call's offsets and result struct: the chained starts, then NO_MESSAGE up to max_m."""
    msg_off, result = got
    have = {k: int(result[k]) for k in RO.RESULT.names}
    assert have == res, "result struct %s, expected %s" % (have, res)
    same(msg_off, np.array(list(offs) + [RO.NO_MESSAGE] * (max_m - len(offs)), dtype=np.uint64), "msg_off")


# ---------------------------------------------------------------- ingest
def refs_tensor(refs):
    import torch

    return torch.from_numpy(np.ascontiguousarray(refs).view(np.uint8).reshape(-1).copy()).cuda()


def fetch_ingest(out_off, out_len, info, wire_crc, total, status):
    return (status.cpu().numpy().view(np.uint32), out_off.cpu().numpy().view(np.uint64),
            out_len.cpu().numpy().view(np.uint64), wire_crc.cpu().numpy().view(np.uint32),
            np.frombuffer(info.cpu().numpy().tobytes(), dtype=IO.INFO), int(total.cpu()[0]))


def run_ingest(messages, wire: bytes, refs, shift=0, oshift=0, version=3, out_cap=None, workspace=None):
    """(status, out_off, out_len, wire_crc, info, total, the output view's bytes): guards checked around the wire
    buffer (which must be unchanged) and the output."""
    import torch

    ww, w = guarded(wire, shift)
    cap = messages.ingest_out_bound(len(wire), len(refs)) if out_cap is None else out_cap
    ow, o = guarded(b"", oshift, cap)
    res = messages.ingest_put_requests_dev(w, refs_tensor(refs), header_version=version, out=o, workspace=workspace)
    torch.cuda.synchronize()
    unchanged(ww, shift, wire, "the wire buffer")
    return fetch_ingest(*res[1:]) + (guards_intact(ow, oshift, cap),)


def assert_ingest_outputs(got, exp):
    """Status, placement, wire CRC, MessageInfo, packed length and every byte of every written span."""
    st, off, ln, crc, info, total, out = got
    est, packed, eoff, eln, ecrc, einfo, etotal = exp
    bad = np.nonzero(st != est)[0]
    assert not len(bad), "request %d: status %#x, expected %#x" % (bad[0], st[bad[0]], est[bad[0]])
    same(off, eoff, "out_off")
    same(ln, eln, "out_len")
    bad = np.nonzero(crc != ecrc)[0]
    assert not len(bad), "request %d: wire CRC %08x, expected %08x" % (bad[0], crc[bad[0]], ecrc[bad[0]])
    same(info, einfo, "info")
    assert total == etotal, "packed length %d, expected %d" % (total, etotal)
    for i, (o, n) in enumerate(zip(eoff, eln)):
        if n:
            o, n = int(o), int(n)
            assert out[o:o + n].tobytes() == packed[o:o + n], "message of request %d differs" % i
    assert (out[etotal:] == 0xA5).all(), "bytes written past the last placed message"


# ---------------------------------------------------------------- k copies of a tile
def copies(tile_dev, k: int):
    """(the whole tensor, the view) of k back-to-back copies of a device tile between guards."""
    whole, view = guarded(k * tile_dev.numel())
    view.copy_(tile_dev.repeat(k))
    return whole, view


def assert_copies(view, tile_dev, k: int, what: str, starts=None):
    """view is k copies of tile_dev, byte for byte; names the first copy, byte and tile message that differ."""
    if tile_dev.numel() == 0 or k == 0:
        return
    ne = view.view(k, -1) != tile_dev
    bad = ne.any(dim=1).cpu().numpy()
    if bad.any():
        c = int(np.nonzero(bad)[0][0])
        b = int(ne[c].nonzero()[0])
        msg = "" if starts is None else ", tile message %d" % (int(np.searchsorted(starts, b, side="right")) - 1)
        raise AssertionError("%s: %d of %d copies differ; first copy %d, byte %d%s: %#x, expected %#x" % (
            what, int(bad.sum()), k, c, b, msg, int(view.view(k, -1)[c, b]), int(tile_dev[b])))


def assert_same(got, exp, what: str):
    """Two numpy arrays, naming the first message that differs."""
    if not np.array_equal(got, exp):
        i = int(np.nonzero(got != exp)[0][0])
        raise AssertionError("%s: %d of %d differ; first message %d (tile message %d): %s, expected %s" % (
            what, int((got != exp).sum()), len(exp), i, i % S.T, got[i], exp[i]))


def offsets_dev(offs, length: int, k: int):
    import torch

    return torch.from_numpy(S.tiled_offsets(offs, length, k)).cuda()
