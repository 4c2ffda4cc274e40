"""Every device entry that reads a stored message's header, over the header lattice (tests/header_lattice.py),
against the oracles test_header_lattice.py holds the CPU entries to: so each equals its CPU twin."""
import numpy as np
import pytest

import hard_delete_oracle as HD
import header_lattice as HL
import recover_oracle as RO
import rekey_oracle as RK
import send_oracle as SO
from gpu_buffers import dev
from gpu_calls import assert_chain, assert_rekey_outputs, check_send, run_hard_delete, run_recover, run_rekey
from header_lattice import rekey_desc, sizes_of
from msgfmt import MF

pytestmark = pytest.mark.gpu


def groups():
    """[(names, region, offsets)]: the packed region as one batch; each truncated region with its lead message."""
    return [HL.packed()] + [([n + "/lead", n], r, [0, o]) for n, r, o in HL.truncated()]


def dev_offs(offs):
    import torch

    return torch.tensor(np.asarray(offs, dtype=np.int64), device="cuda")


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["jobs", "region", "region2"])
def test_verify(gpu, mode):
    import torch

    gpu.set_region_mode(0, mode)
    try:
        for names, region, offs in groups():
            status, end = gpu.verify_messages(dev(region), dev_offs(offs))
            torch.cuda.synchronize()
            got = list(zip(status.cpu().numpy().view(np.uint32).tolist(), end.cpu().numpy().tolist()))
            assert got == [MF.verify_message(region, o) for o in offs], names[-1]
    finally:
        gpu.set_region_mode(0, 2)


def test_verify_host_gpu_leg(gpu):
    for names, region, offs in groups():
        st, end = gpu.verify_messages_host(region, offs)
        assert gpu.last_host_path(0) == 1
        assert [(int(s), int(e)) for s, e in zip(st, end)] == [MF.verify_message(region, o) for o in offs], names[-1]


def test_transform(gpu):
    import torch

    from ambry_amd.messages import transform_dev

    for names, region, offs in groups():
        for version, use_life in ((3, True), (3, False), (1, True)):
            life = (np.arange(len(offs)) % 5).astype(np.int16)
            out, out_off, out_len, status = transform_dev(
                dev(region), dev_offs(offs), header_version=version,
                life_version=torch.from_numpy(life).cuda() if use_life else None)
            torch.cuda.synchronize()
            # the lattice breaks the fast path's premise (dense clean V3 PUTs): it must have refused the batch
            assert gpu.last_transform_path(0) == 0, names[-1]
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


def test_hard_delete(gpu):
    for names, region, offs in groups():
        exp = HD.hard_delete(region, offs)
        for plan_only in (True, False):
            st, info, after = run_hard_delete(gpu, region, offs, shift=3, plan_only=plan_only)
            assert st == exp[0], names[-1]
            assert np.array_equal(info, exp[1]), names[-1]
            assert after == (region if plan_only else exp[2]), names[-1]


def test_rekey(gpu):
    from ambry_amd import messages

    d, aux = rekey_desc()
    for names, region, offs in groups():
        descs = np.repeat(np.asarray([d], dtype=RK.DESC), len(offs))
        for version, life in ((3, None), (1, [4] * len(offs))):
            exp = RK.expected(region, offs, descs, aux, life=life, version=version)
            assert_rekey_outputs(run_rekey(messages, region, offs, descs, aux, shift=5, life=life, version=version), exp)


@pytest.mark.parametrize("sized", [False, True], ids=["header-size", "given-size"])
def test_send(gpu, sized):
    from ambry_amd import messages

    for names, region, offs in groups():
        sizes = sizes_of(region, offs) if sized else None
        for flag in SO.FLAGS:
            check_send(messages, region, offs, sizes, flag, shift=1, slack=3)


def test_chain_and_recover(gpu):
    names, region, offs = HL.packed()
    starts = [(region, o) for o in offs] + [(r, o) for _, r, o in HL.truncated() if o <= len(r)]
    for region, start in starts:
        RO.assert_call(run_recover(gpu, region, start, 3), RO.recover(region, start, 3), 3)
        assert_chain(run_recover(gpu, region, start, 3, chain=True), *RO.chain_result(region, start, 3), 3)
