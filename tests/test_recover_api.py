"""CPU: the surface of bzh_recover* -- the header, SIGNATURES and the library agree on the five functions, the entry is 48
bytes, null handles are refused, the Python entry points check their arguments before any context is made, and bnzhip knows
--recover and refuses it beside a level or --decompress without asking for a device."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "banzai_amd", "bnzhip")
NEW = ("bzh_recover_device", "bzh_recover", "bzh_get_recover_stats", "bzh_recover_stream_device", "bzh_recover_stream")


def test_header_signatures_and_library_agree(native):
    text = open(os.path.join(ROOT, "include", "bzhip.h")).read()
    declared = set(re.findall(r"BZH_API[^;(]*?\b(bzh_\w+)\s*\(", text))
    L = ctypes.CDLL(native.LIB_PATH)
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/bzhip.h"
        assert name in native.SIGNATURES, f"{name} is missing from SIGNATURES"
        assert hasattr(L, name), f"{name} is not exported"
    assert native.MISSING == []
    for word in ("bzh_recover_entry", "bzh_recover_stats", "BZH_REC_JOINED", "BZH_REC_STREAM_END", "BZH_REC_STREAM_OK", "shadowed", "streams_ok"):
        assert word in text, word
    assert len(native.SIGNATURES["bzh_recover_device"][1]) == 9 and len(native.SIGNATURES["bzh_recover"][1]) == 9
    assert len(native.SIGNATURES["bzh_recover_stream_device"][1]) == 8 and len(native.SIGNATURES["bzh_recover_stream"][1]) == 8


def test_entry_and_stats_layout(native):
    assert ctypes.sizeof(native.RecoverEntry) == 48 and native.RECOVER_DTYPE.itemsize == 48
    assert [f[0] for f in native.RecoverEntry._fields_] == list(native.RECOVER_DTYPE.names)
    for name, _ in native.RecoverEntry._fields_:
        assert getattr(native.RecoverEntry, name).offset == native.RECOVER_DTYPE.fields[name][1], name
    assert ctypes.sizeof(native.RecoverStats) == 64
    text = open(os.path.join(ROOT, "include", "bzhip.h")).read()
    for name, value in (("BZH_REC_JOINED", native.REC_JOINED), ("BZH_REC_STREAM_END", native.REC_STREAM_END),
                        ("BZH_REC_STREAM_OK", native.REC_STREAM_OK), ("BZH_LOST_TRUNC", native.LOST_TRUNC),
                        ("BZH_LOST_FORMAT", native.LOST_FORMAT), ("BZH_LOST_BLOCK_CRC", native.LOST_BLOCK_CRC),
                        ("BZH_LOST_RANDOMISED", native.LOST_RANDOMISED)):
        assert re.search(rf"\b{name} = {value}\b", text), name


def test_null_handles_are_refused(native):
    L = native.lib()
    st = native.RecoverStats()
    n = ctypes.c_size_t(0)
    assert L.bzh_get_recover_stats(None, ctypes.byref(st)) == -1
    assert L.bzh_recover_device(None, None, 0, None, 0, ctypes.byref(n), None, 0, ctypes.byref(n)) == -1
    assert L.bzh_recover(None, None, 0, None, 0, ctypes.byref(n), None, 0, ctypes.byref(n)) == -1
    assert L.bzh_recover_stream_device(None, None, 0, None, 0, None, 0, ctypes.byref(n)) == -1
    assert L.bzh_recover_stream(None, None, 0, None, 0, None, 0, ctypes.byref(n)) == -1


def test_python_argument_checks_come_first():
    """type checks raise before a context (and with it a device) is asked for"""
    import banzai_amd
    assert "recover" in banzai_amd.__all__ and "recover_stream" in banzai_amd.__all__
    for bad in ("text", 7, None, [b"x"]):
        with pytest.raises(TypeError):
            banzai_amd.recover(bad)
        with pytest.raises(TypeError):
            banzai_amd.recover_stream(bad)
    for bad in (5, "report", b"bytes", {"a": 1}):
        with pytest.raises(TypeError):
            banzai_amd.recover_stream(b"BZh9", report=bad)


def test_recovered_views():
    """Recovered's kept / lost / complete are host arithmetic over the blocks"""
    from banzai_amd import Recovered, RecoveredBlock, _native
    J, E, K = _native.REC_JOINED, _native.REC_STREAM_END, _native.REC_STREAM_OK
    a = RecoveredBlock(32, 500, 0, 10, 1, 0, J, 0)
    b = RecoveredBlock(500, 900, 10, 10, 2, 0, J | E | K, 0)
    lost = RecoveredBlock(500, 0, 10, 0, 2, _native.LOST_BLOCK_CRC, 0, 500)
    r = Recovered(b"x" * 20, [a, b], {})
    assert r.complete and r.kept == [a, b] and r.lost == []
    assert not Recovered(b"x" * 10, [a, lost], {}).complete and Recovered(b"", [a, lost], {}).lost == [lost]
    assert not Recovered(b"", [a, b._replace(flags=J | E)], {}).complete      # the footer does not check out
    assert not Recovered(b"", [a._replace(flags=0), b], {}).complete          # the first block hangs on no header
    assert not Recovered(b"", [a], {}).complete                               # the run ends in no footer
    assert Recovered(b"", [], {}).complete


def test_cli_knows_recover_and_its_argument_errors():
    """--help names it; beside a level option or --decompress it is an argument error, code 1, before any device is asked for"""
    r = subprocess.run([BIN, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--recover" in r.stderr and "4 (salvage" in r.stderr
    for extra in (["-d"], ["--decompress"], ["-1"], ["-9"], ["--fast"], ["--best"], ["-k5"]):
        r = subprocess.run([BIN, "--recover", *extra, "nothing.bz2"], capture_output=True, text=True)
        assert r.returncode == 1, (extra, r.returncode, r.stderr)
        r = subprocess.run([BIN, *extra, "--recover", "nothing.bz2"], capture_output=True, text=True)
        assert r.returncode == 1, (extra, r.returncode, r.stderr)
