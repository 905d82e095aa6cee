"""Lane checkpoints and map import without a GPU: the new entry points are declared and exported (the ABI version stays 3), and
ll_checkpoint_describe -- pure host code -- accepts hand-built blobs of the documented layout and refuses broken
ones with LL_ERR_ARG."""
import ctypes as C
import struct

import numpy as np
import pytest

from test_cabi import declared_symbols

NEW = ["ll_cubemaps_layout", "ll_cubemaps_import", "ll_cubemap_layout", "ll_cubemap_import",
       "ll_drives_save_size", "ll_drives_save", "ll_drives_restore", "ll_checkpoint_describe"]
MAGIC, VERSION, HEADER, RECORD = 0x4B434C4C, 1, 64, 96
N_CUBES = 4851
COUNTS_BYTES = (2 * N_CUBES * 4 + 15) // 16 * 16
TAB_BYTES = COUNTS_BYTES + 512
STATE_BYTES = 11 * 16                      # slot pose, odom, map-to-odom [7] doubles each, the frame counter
HEADER_BOUNDARIES = [0, 4, 8, 12, 16, 24, 28, 32, 36, 40, 44, 48, 52, 56, 60]   # the first byte of every header field


def header(n_records=0, total=HEADER, magic=MAGIC, version=VERSION, n_scans=16, need=(0, 0, 0, 0)):
    h = struct.pack("<4IQI3i2f4i", magic, version, HEADER, RECORD, total, n_records, n_scans, 0, 0, 0.4, 0.8, *need)
    assert len(h) == HEADER
    return h


def one_record_blob(offset=None, tab_offset=None):
    """one lane with an empty map and empty feature clouds: header, record, counts + valid list, 11 points of state"""
    tab = HEADER + RECORD
    dev = (tab + TAB_BYTES + 255) // 256 * 256
    total = dev + STATE_BYTES
    rec = struct.pack("<3Q2q14i", tab if tab_offset is None else tab_offset, dev if offset is None else offset, STATE_BYTES,
                      0, 0, 2, 7, 10, 10, 5, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    assert len(rec) == RECORD
    body = bytearray(total)
    body[:HEADER] = header(1, total)
    body[HEADER:HEADER + RECORD] = rec
    return bytes(body)


def test_new_symbols_are_declared_and_exported(api):
    lib = api.load_library()
    syms = declared_symbols()
    for s in NEW:
        assert s in syms, f"{s} is not declared in lightloam_hip.h"
        assert hasattr(lib, s), f"{s} is not exported by the library"
        assert s in api.EXPORTS
    assert lib.ll_abi_version() == 3


def test_describe_accepts_a_minimal_blob(api):
    info = api.describe_checkpoint(header())
    assert (info["version"], info["n_records"], info["total_bytes"], info["n_scans"]) == (1, 0, 64, 16)
    assert info["line_res"] == np.float32(0.4) and info["plane_res"] == np.float32(0.8) and info["records"] == []
    info = api.describe_checkpoint(one_record_blob())
    assert info["n_records"] == 1
    r = info["records"][0]
    assert (r["lane"], r["frame_index"], r["n_corner"], r["n_surf"], r["n_features"], r["bytes"]) == (2, 7, 0, 0, (0, 0, 0, 0), STATE_BYTES)


def _refused(api, blob):
    with pytest.raises(api.LightLoamError) as e:
        api.describe_checkpoint(blob)
    return e.value.code == -2


def test_describe_refuses_broken_blobs(api):
    assert _refused(api, header(magic=MAGIC ^ 1))
    assert _refused(api, header(magic=0x4C4C434B))                  # the bytes of the magic the other way round
    assert _refused(api, header(version=VERSION + 1))
    assert _refused(api, header(version=0))
    good = header()
    for cut in HEADER_BOUNDARIES:
        assert _refused(api, good[:cut]), cut
    assert _refused(api, good + b"\0" * 16)                          # bytes disagrees with total_bytes
    assert _refused(api, header(n_records=1))                        # the record table runs past the end
    blob = one_record_blob()
    assert _refused(api, blob[:-16])                                 # truncated inside the payload
    assert _refused(api, one_record_blob(offset=len(blob)))          # a record offset past the end of the blob
    assert _refused(api, one_record_blob(offset=len(blob) + (1 << 40)))
    assert _refused(api, one_record_blob(tab_offset=len(blob)))      # the counts past the end
    assert _refused(api, one_record_blob(tab_offset=HEADER))          # the counts over the record table
    assert _refused(api, one_record_blob(offset=HEADER + RECORD + 16))   # the payload over the counts
    bad = bytearray(blob); struct.pack_into("<i", bad, HEADER + RECORD + 4 * 17, 3)   # a cube count the record's n_pts does not cover
    assert _refused(api, bytes(bad))


def test_describe_needs_no_context(api):
    """the raw call: NULL arguments are LL_ERR_ARG, and nothing of it touches a device"""
    lib = api.load_library()
    info = api.CheckpointInfo()
    assert lib.ll_checkpoint_describe(None, 64, C.addressof(info)) == -2
    raw = np.frombuffer(header(), np.uint8)
    assert lib.ll_checkpoint_describe(raw.ctypes.data, raw.size, None) == -2
    assert lib.ll_checkpoint_describe(raw.ctypes.data, raw.size, C.addressof(info)) == 0 and info.n_records == 0
