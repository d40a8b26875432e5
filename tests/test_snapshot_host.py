"""The host side of a context snapshot, without a GPU: grlx_snapshot_info on malformed input, the device entry points without a
device, and the stand-alone run of the header's reader under the host sanitizers (tools/snapshot_format_check.cpp: host code compiled
from the HIP-free format file, run on the CPU as a program of its own)."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMAT = os.path.join(ROOT, "grl_amd", "csrc", "grlx_snapshot_format.cpp")
CHECK = os.path.join(ROOT, "tools", "snapshot_format_check.cpp")


def _fnv1a(data, h=0xcbf29ce484222325):
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def _reseal(header: bytes) -> bytes:
    """the header with its own checksum (bytes 32..39, computed with those bytes as zero) made right again"""
    body = header[:32] + bytes(8) + header[40:]
    return header[:32] + struct.pack("<Q", _fnv1a(body)) + header[40:]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """the stand-alone program, built once with the host sanitizers (their runtimes linked statically: the program carries its own and
    starts in whatever environment the suite runs in); run, it also writes a valid header"""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tools/snapshot_format_check.cpp")
    d = tmp_path_factory.mktemp("snapshot_format")
    exe = str(d / "snapshot_format_check")
    res = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                          CHECK, FORMAT, "-o", exe],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe, str(d / "header.bin")


def test_stand_alone_parser_run_under_the_host_sanitizers(checker):
    exe, header = checker
    res = subprocess.run([exe, header], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "refused" in res.stdout and "ERROR" not in res.stderr and "runtime error" not in res.stderr, res.stderr


@pytest.fixture(scope="module")
def valid_header(checker):
    exe, header = checker
    if not os.path.exists(header):
        res = subprocess.run([exe, header], capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stdout + res.stderr
    with open(header, "rb") as f:
        return f.read()


def _info(grlx, data):
    info = grlx.capi.SnapshotInfo()
    rc = grlx.capi.load().grlx_snapshot_info(bytes(data), len(data), C.byref(info))
    return rc, grlx.capi.load().grlx_last_error().decode(), info


def test_info_reads_a_valid_header(grlx, valid_header):
    rc, msg, info = _info(grlx, valid_header)
    assert rc == grlx.capi.OK, msg
    assert (info.format_version, info.n_replicas, info.n_tables, info.table_log2, info.trials_run) == (1, 13, 2, 13, 12)
    assert (info.is_sweep, info.has_trace, info.has_target, info.twin_tables, info.rows, info.record_bytes) == (0, 1, 0, 1, 1, 24)
    assert info.header_bytes == len(valid_header) and info.n_records == 4321 and info.checksum == 0x0123456789abcdef
    assert list(info.section_bytes) == [13 * 256, 4 * 8 * 13, 13 * 16 * 10 * 2 * 4, 0, 4321 * 24]
    assert info.total_bytes == info.header_bytes + sum(info.section_bytes)
    assert info.config.struct_size == C.sizeof(grlx.capi.Config) and info.config.n_replicas == 13 and info.config.alpha == 0.2
    assert grlx.snapshot_info(valid_header).n_records == 4321          # the Python entry takes bytes or a path


def test_info_refuses_empty_garbage_and_truncated_input(grlx, valid_header):
    capi = grlx.capi
    for data in (b"", b"\0" * 7, b"not a snapshot at all, just some text" * 40, os.urandom(len(valid_header)), valid_header[:-1], valid_header[:64], valid_header[:16]):
        rc, msg, _ = _info(grlx, data)
        assert rc == capi.ERR_INVALID and msg, (len(data), msg)
    info = capi.SnapshotInfo()
    assert capi.load().grlx_snapshot_info(None, 0, C.byref(info)) == capi.ERR_INVALID
    assert capi.load().grlx_snapshot_info(valid_header, len(valid_header), None) == capi.ERR_INVALID
    with pytest.raises(capi.GrlxError):
        grlx.snapshot_info(b"garbage")


# (offset, struct format, corrupted value, a word of the message) -- the layout of grl_amd/csrc/grlx_snapshot_format.h; the header
# checksum is made right again after each, so that the field's own validation answers
FIELDS = [("magic", 0, "<8s", b"GRLXSNAQ", "magic"), ("version 0", 8, "<I", 0, "version"), ("newer version", 8, "<I", 2, "newer"),
          ("header bytes", 12, "<I", 800, "header"), ("total bytes", 16, "<Q", 12345, "total"), ("n_replicas", 40, "<I", 14, "n_replicas"),
          ("n_replicas 0", 40, "<I", 0, "n_replicas"), ("n_tables", 44, "<I", 3, "n_tables"), ("capacity", 48, "<I", 27, "capacity"),
          ("flags", 52, "<I", 1 << 9, "flags"), ("trace flag off", 52, "<I", 8, "section"), ("trials_run", 56, "<q", -1, "trial"),
          ("rows", 64, "<I", 25, "rows"), ("record bytes", 68, "<I", 32, "record"), ("states section", 72, "<Q", 13 * 256 + 8, "section"),
          ("rows section", 80, "<Q", 0, "section"), ("trace section", 88, "<Q", 0, "section"), ("sweep section", 96, "<Q", 8, "section"),
          ("records section", 104, "<Q", 4320 * 24, "section"), ("record count", 112, "<Q", 1 << 40, "records"), ("state bytes", 120, "<I", 240, "state"),
          ("abi", 124, "<I", 1, "ABI"), ("struct_size", 128, "<I", 12, "struct_size")]


@pytest.mark.parametrize("name,offset,fmt,value,word", FIELDS, ids=[f[0] for f in FIELDS])
def test_info_refuses_every_corrupted_field(grlx, valid_header, name, offset, fmt, value, word):
    n = struct.calcsize(fmt)
    bad = valid_header[:offset] + struct.pack(fmt, value) + valid_header[offset + n:]
    rc, msg, _ = _info(grlx, bad)                               # as it is: the header checksum catches it (or the magic / version before it)
    assert rc == grlx.capi.ERR_INVALID and msg
    rc, msg, _ = _info(grlx, _reseal(bad))                      # under a right checksum: the field's own check
    assert rc == grlx.capi.ERR_INVALID and word in msg, msg


def test_info_refuses_a_damaged_header_checksum_and_payload_free_changes(grlx, valid_header):
    for at in (24, 33, 130, len(valid_header) - 1):            # the payload checksum field, the header checksum, the configuration, the padding
        bad = bytearray(valid_header)
        bad[at] ^= 0x40
        rc, msg, _ = _info(grlx, bad)
        assert rc == grlx.capi.ERR_INVALID and "checksum" in msg, msg


def test_device_entry_points_without_a_device(grlx, valid_header):
    capi = grlx.capi
    lib = capi.load()
    if lib.grlx_device_count() > 0:
        pytest.skip("a GPU is present")
    n = C.c_uint64(0)
    buf = (C.c_ubyte * 64)()
    assert lib.grlx_snapshot_size(None, C.byref(n)) == capi.ERR_NO_DEVICE
    assert lib.grlx_snapshot_save(None, buf, 64, C.byref(n)) == capi.ERR_NO_DEVICE
    assert lib.grlx_snapshot_load(None, valid_header, len(valid_header)) == capi.ERR_NO_DEVICE
    assert "no HIP device" in lib.grlx_last_error().decode()
