"""What the per-feature oracles (send, receive, re-key, ingest, recover, hard delete) share: the status bits the
message entries add to oracle/message_format.py's, the sentinels and record shapes of the ABI, a record's CRC
against its stored long, Java's expiry arithmetic and the packed placement of a batch's outputs.

The oracles stay independent of the library: every constant here is a literal restated from include/ambrycrc.h,
not imported from ambry_amd.abi. The dtype assertions in the tests' fixtures (M.SEND_INFO_DTYPE == SO.INFO and
the like) and test_abi_mirror.py tie the two together."""
import struct
import zlib

import numpy as np

from msgfmt import MF

# status bits beyond MF's
NO_ROOM = 1 << 12
NEEDS_CONTENT = 1 << 14
BAD_DESC = 1 << 15
BAD_INFO = 1 << 16
WIRE_CRC = 1 << 17
BAD_RANGE = 1 << 18

NOWHERE = 0xFFFFFFFFFFFFFFFF  # out_off of a message not written
INT_MAX = 0x7FFFFFFF
LONG_MAX, LONG_MIN = (1 << 63) - 1, -(1 << 63)

BLOB_HEAD = {1: 10, 2: 12, 3: 13}  # blob record version -> bytes before the content
MESSAGE_INFO = np.dtype([("msg_off", "<u8"), ("size", "<u8"), ("expires_at_ms", "<i8"), ("operation_time_ms", "<i8"),
                         ("key_rel", "<u4"), ("key_len", "<u4"), ("account_id", "<i2"), ("container_id", "<i2"),
                         ("life_version", "<i2"), ("flags", "u1"), ("header_version", "u1")])


# ---------------------------------------------------------------- comparing a batch's answers
def same(got, exp, what: str):
    """got == exp for two lists, byte strings or numpy arrays (a structured array field by field); a failure names
    `what`, how many elements differ and the first of them with both values."""
    names = getattr(getattr(exp, "dtype", None), "names", None)
    if names:
        for name in names:
            same(np.asarray(got)[name], exp[name], "%s, field %s" % (what, name))
        return
    if isinstance(exp, (bytes, bytearray)):
        got, exp = np.frombuffer(bytes(got), dtype=np.uint8), np.frombuffer(exp, dtype=np.uint8)
    if isinstance(got, np.ndarray) and isinstance(exp, np.ndarray):
        assert got.shape == exp.shape, "%s: shape %s, expected %s" % (what, got.shape, exp.shape)
        bad = np.nonzero(got != exp)[0]
    else:  # lists of Python integers: compared as such, UINT64_MAX among small values included
        got, exp = list(got), list(exp)
        assert len(got) == len(exp), "%s: %d elements, expected %d" % (what, len(got), len(exp))
        bad = [i for i, (g, e) in enumerate(zip(got, exp)) if g != e]
    assert not len(bad), "%s: %d of %d differ; first at %d: %s, expected %s" % (what, len(bad), len(exp), bad[0],
                                                                               got[bad[0]], exp[bad[0]])


# ---------------------------------------------------------------- records
def crc_bad(region: bytes, lo: int, hi: int) -> bool:
    """Record [lo, hi) of the region: the CRC of all but its last 8 bytes against the big-endian long they hold."""
    return zlib.crc32(region[lo:hi - 8]) != struct.unpack_from(">Q", region, hi - 8)[0]


def flip(b: bytes, at: int, bit=0x40) -> bytes:
    return b[:at] + bytes([b[at] ^ bit]) + b[at + 1:]


def refit(msg: bytes, lo: int, hi: int, edit) -> bytes:
    """msg with record [lo, hi) edited (edit(bytearray of the record)) and its CRC trailer recomputed."""
    rec = bytearray(msg[lo:hi])
    edit(rec)
    rec[-8:] = MF._crc_long(bytes(rec[:-8]))
    return msg[:lo] + bytes(rec) + msg[hi:]


# ---------------------------------------------------------------- Java's time arithmetic
def wrap64(x: int) -> int:
    """A Java long after an add that may overflow."""
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


def seconds_to_millis(d: int) -> int:
    """TimeUnit.SECONDS.toMillis: saturates at Long.MAX_VALUE / Long.MIN_VALUE."""
    over = LONG_MAX // 1000
    return LONG_MAX if d > over else LONG_MIN if d < -over else d * 1000


def add_seconds_to_epoch(epoch_ms: int, delta_s: int) -> int:
    """Utils.addSecondsToEpochTime (Utils.java:1036-1041): toMillis saturates, the add wraps."""
    if epoch_ms == -1 or delta_s == -1:
        return -1
    return wrap64(epoch_ms + seconds_to_millis(delta_s))


# ---------------------------------------------------------------- the packed placement
def place_packed(lengths, out_cap=None):
    """Where each output of a batch goes: outputs in message order from 0. lengths[i] is the output's length, or
    None for a message that has none. Returns a list: the output's offset, or None for a message without an output
    and for one whose span ends past out_cap -- which gets NO_ROOM from the caller but still advances the running
    offset, so a later, shorter output is refused too unless it fits below out_cap at its own place."""
    at, pos = [], 0
    for n in lengths:
        if n is None:
            at.append(None)
            continue
        at.append(pos if out_cap is None or pos + n <= out_cap else None)
        pos += n
    return at
