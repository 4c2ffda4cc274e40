"""ambry_amd -- MI355X-native engine for Ambry's blob CRC-32 path.

Layers:
  include/ambrycrc.h + ambry_amd/csrc/   C ABI and gfx950 kernels (libambrycrc.so)
  ambry_amd.abi                          the header's constants and structs, mirrored once
  ambry_amd._lib                         ctypes signatures of every exported symbol; the loader
  ambry_amd._args                        the wrappers' argument layer: tensor check, pointer, stream, host buffer
  ambry_amd.crc32                        mirror of com.github.ambry.utils.Crc32 (host path)
  ambry_amd.device                       device-resident batch / verify / hard delete / recovery over torch HBM
  ambry_amd.messages                     PUT serialization, transform, re-key, ingest, GET send and receive
  ambry_amd.multi                        one-process-per-GPU sharding + RCCL all-gather
"""
from ._lib import EXPORTED, LIB_PATH, AmbryCrcError, lib  # noqa: F401
from .crc32 import Crc32, combine, crc32, zeros  # noqa: F401

__all__ = ["Crc32", "crc32", "combine", "zeros", "lib", "LIB_PATH", "EXPORTED", "AmbryCrcError"]
