"""CPU: the decoder's public surface without a device -- what the header declares, argument checks of the Python layer, the
loud failure on a box without a GPU, and the compiler's resource report for the decode translation unit."""
import io
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_decoder():
    text = open(os.path.join(ROOT, "include", "bzhip.h")).read()
    syms = set(re.findall(r"BZH_API[^;(]*?\b(bzh_\w+)\s*\(", text))
    for need in ("bzh_decode", "bzh_decode_device", "bzh_get_decode_stats", "bzh_decode_scan"):
        assert need in syms
    assert re.search(r"BZH_E_DATA\s*=\s*-6", text)
    assert "bzh_decode_stats" in text and "candidates_off_chain" in text
    assert "randomised" in text.lower()  # the header says that randomised blocks are refused


def test_bindings_mirror_the_header(native):
    assert native.MISSING == []
    for name in ("bzh_decode", "bzh_decode_device", "bzh_get_decode_stats", "bzh_decode_scan"):
        assert name in native.SIGNATURES
    assert native.lib().bzh_strerror(-6) == b"not a valid bzip2 stream"
    # six doubles and six 64-bit counters, the layout of bzh_decode_stats
    import ctypes
    assert ctypes.sizeof(native.DecodeStats) == 96
    for attr in ("decode", "decode_scan", "decode_stats", "decode_device"):
        assert hasattr(native.Context, attr)


def test_python_surface_rejects_non_bytes():
    import banzai_amd
    assert "decompress" in banzai_amd.__all__ and "decode" in banzai_amd.__all__
    for bad in ("text", 5, None, 3.5, ["x"]):
        with pytest.raises(TypeError):
            banzai_amd.decompress(bad)

    class TextReader:
        def read(self):
            return "not bytes"
    with pytest.raises(TypeError):
        banzai_amd.decode(TextReader(), io.BytesIO())


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.skipif(_have_gpu(), reason="only meaningful on a box without a GPU")
def test_no_gpu_fails_loudly(native):
    import bz2
    import banzai_amd
    s = bz2.compress(b"abc")
    with pytest.raises(native.BzhError) as e:
        banzai_amd.decompress(s)
    assert e.value.status == -3
    with pytest.raises(native.BzhError) as e:
        banzai_amd.decode(io.BytesIO(s), io.BytesIO())
    assert e.value.status == -3


def test_decode_kernels_use_no_scratch_memory():
    """scripts/resource_usage.py on decode.hip: no decode kernel may spill or use scratch memory (the project's standing
    rule; tests/test_abi.py lists its translation units by name and does not see this one)"""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import resource_usage
    kernels = resource_usage.report(os.path.join(ROOT, "banzai_amd", "csrc", "decode.hip"))
    names = " ".join(k["name"] for k in kernels)
    for need in ("decode_scan_kernel", "decode_block_kernel", "unrle_maps", "unrle_walk"):
        assert need in names
    bad = [(r["name"], r.get("VGPRs Spill"), r.get("ScratchSize [bytes/lane]")) for r in kernels
           if r.get("ScratchSize [bytes/lane]", "0") != "0" or r.get("VGPRs Spill", "0") != "0"]
    assert not bad, bad


def test_cli_help_names_the_option(native):
    import subprocess
    r = subprocess.run([os.path.join(ROOT, "banzai_amd", "bnzhip"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--decompress" in r.stderr and "-d" in r.stderr
    # argument errors of the decode direction need no device
    r = subprocess.run([os.path.join(ROOT, "banzai_amd", "bnzhip"), "-d", os.path.join(ROOT, "README.md")], capture_output=True)
    assert r.returncode == 1
