"""Two faults in one message through every device entry that reads a stored message (header_lattice.pairs():
about 6,400 messages as one batch a call; truncated_pairs(): a call a region), against the oracles
test_pair_lattice.py holds the CPU entries to. Every buffer sits between guards, and a refused message must be
byte for byte as it was."""
import numpy as np
import pytest

import hard_delete_oracle as HD
import header_lattice as HL
import recover_oracle as RO
import rekey_oracle as RK
import send_oracle as SO
from gpu_buffers import assert_untouched, guarded
from gpu_calls import (assert_chain, assert_rekey_outputs, check_send, recover_to_numpy, run_hard_delete, run_recover,
                       run_rekey, unchanged)
from header_lattice import pair_descs, sizes_of
from msgfmt import MF
from oracle_common import same

pytestmark = pytest.mark.gpu


def dev_offs(offs):
    import torch

    return torch.tensor(np.asarray(offs, dtype=np.int64), device="cuda")


def run_verify(gpu, region, offs, shift):
    import torch

    whole, r = guarded(region, shift)
    status, end = gpu.verify_messages(r, dev_offs(offs))
    torch.cuda.synchronize()
    assert_untouched(whole, r, region, shift)
    return list(zip(status.cpu().numpy().view(np.uint32).tolist(), end.cpu().numpy().tolist()))


def first_difference(names, got, exp):
    """None, or the first case whose answers differ, by name."""
    for n, g, e in zip(names, got, exp):
        if g != e:
            return "%s: %s, expected %s" % (n, g, e)
    assert len(got) == len(exp)
    return None


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["jobs", "region", "region2"])
def test_verify(gpu, mode):
    names, region, offs = HL.pairs()
    exp = [MF.verify_message(region, o) for o in offs]
    gpu.set_region_mode(0, mode)
    try:
        got = run_verify(gpu, region, offs, shift=3)
        assert gpu.last_message_mode(0) == mode
    finally:
        gpu.set_region_mode(0, 2)
    assert first_difference(names, got, exp) is None


def test_verify_host_gpu_leg(gpu):
    names, region, offs = HL.pairs()
    st, end = gpu.verify_messages_host(region, offs)
    assert gpu.last_host_path(0) == 1
    got = [(int(s), int(e)) for s, e in zip(st, end)]
    assert first_difference(names, got, [MF.verify_message(region, o) for o in offs]) is None


@pytest.mark.parametrize("version,use_life", [(3, True), (3, False), (1, True)], ids=["v3-life", "v3", "v1-life"])
def test_transform(gpu, version, use_life):
    import torch

    from ambry_amd.messages import transform_dev

    names, region, offs = HL.pairs()
    life = (np.arange(len(offs)) % 5).astype(np.int16)
    whole, r = guarded(region, 3)
    out, out_off, out_len, status = transform_dev(r, dev_offs(offs), header_version=version,
                                                  life_version=torch.from_numpy(life).cuda() if use_life else None)
    torch.cuda.synchronize()
    assert gpu.last_transform_path(0) == 0  # the fast path's premise (dense clean V3 PUTs) does not hold
    assert_untouched(whole, r, region, 3)
    out_h = out.cpu().numpy().tobytes()
    st, oo, ol = status.cpu().numpy().view(np.uint32), out_off.cpu().numpy(), out_len.cpu().numpy()
    pos = 0
    for i, o in enumerate(offs):
        est, exp = MF.transform_message(region, o, life=int(life[i]) if use_life else None, version=version)
        assert int(st[i]) == est, names[i]
        if exp is None:
            assert ol[i] == 0 and oo[i] == -1, names[i]
            continue
        assert oo[i] == pos and ol[i] == len(exp) and out_h[pos:pos + len(exp)] == exp, names[i]
        pos += len(exp)


@pytest.mark.parametrize("plan_only", [True, False], ids=["plan", "delete"])
def test_hard_delete(gpu, plan_only):
    names, region, offs = HL.pairs()
    est, einfo, eafter = HD.hard_delete(region, offs)
    assert 0 < sum(1 for s in est if s == 0) < len(est) // 4  # deleted although another record is at fault
    st, info, after = run_hard_delete(gpu, region, offs, shift=3, plan_only=plan_only)
    assert first_difference(names, st, est) is None
    same(info, einfo, "info")
    same(after, region if plan_only else eafter, "the region afterwards")


@pytest.mark.parametrize("version,life", [(3, None), (1, 4)], ids=["v3", "v1-life"])
def test_rekey(gpu, version, life):
    from ambry_amd import messages

    names, region, offs = HL.pairs()
    descs, aux = pair_descs(len(offs))
    life = None if life is None else [life] * len(offs)
    exp = RK.expected(region, offs, descs, aux, life=life, version=version)
    got = run_rekey(messages, region, offs, descs, aux, shift=5, life=life, version=version)
    assert first_difference(names, got[0], exp[0]) is None
    assert_rekey_outputs(got, exp)


@pytest.mark.parametrize("sized", [False, True], ids=["header-size", "given-size"])
@pytest.mark.parametrize("flag", SO.FLAGS)
def test_send(gpu, flag, sized):
    from ambry_amd import messages

    names, region, offs = HL.pairs()
    check_send(messages, region, offs, sizes_of(region, offs) if sized else None, flag, shift=1, slack=3)


def test_chain_and_recover(gpu):
    """Started where header_lattice.recover_starts() says (a start is a call; its docstring says how they are
    chosen), three messages a call: so a start also reads the two cases behind it, where its own header is intact."""
    names, region, offs = HL.pairs()
    starts = HL.recover_starts()
    assert len(starts) < 700
    whole, r = guarded(region, 3)  # one guarded copy for every start: checked unchanged once, at the end
    for i in starts:
        RO.assert_call(recover_to_numpy(gpu.recover_messages(r, offs[i], 3)), RO.recover(region, offs[i], 3), 3)
        assert_chain(recover_to_numpy(gpu.chain_messages(r, offs[i], 3)), *RO.chain_result(region, offs[i], 3), 3)
    unchanged(whole, 3, region, "the region")


def test_truncated_pairs(gpu):
    """The regions that end inside a twice-faulted message, a call a region: the verify, the send under ALL (with
    the header's size and with the size up to the region's end) and recover."""
    from ambry_amd import messages

    for name, region, off in HL.truncated_pairs():
        offs = [0, off]
        got = run_verify(gpu, region, offs, shift=1)
        assert got == [MF.verify_message(region, o) for o in offs], name
        for sizes in (None, sizes_of(region, offs)):
            check_send(messages, region, offs, sizes, SO.ALL, shift=1, slack=3)
        RO.assert_call(run_recover(gpu, region, off, 3), RO.recover(region, off, 3), 3)
