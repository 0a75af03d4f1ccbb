"""The host engine as a set of translation units (csrc/saip_engine*.cpp), no GPU needed: the shared object exports exactly the C-ABI of
include/saip.h -- no entry lost between the units, no internal helper exported under an unmangled saip_ name -- and every file under
csrc/ is on the build lists of capi.py, whose header list decides when a stale libsaip.so is rebuilt."""
import glob
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sai-primitives_amd")


@pytest.fixture(scope="module")
def sp():
    import sai_primitives_amd as sp
    sp.build_library()
    return sp


def _nm():
    for tool in ("nm", "llvm-nm"):
        if shutil.which(tool):
            return shutil.which(tool)
    hipcc = shutil.which("hipcc")  # llvm-nm of the ROCm tree the library was built with
    for rel in ("../llvm/bin/llvm-nm", "../lib/llvm/bin/llvm-nm"):
        cand = os.path.join(os.path.dirname(os.path.realpath(hipcc)), rel) if hipcc else ""
        if os.path.exists(cand):
            return cand
    raise AssertionError("neither nm nor llvm-nm found")


def test_exported_saip_symbols_are_the_declared_c_abi(sp):
    L = sp.lib()
    out = subprocess.run([_nm(), "-D", "--defined-only", os.path.join(PKG, "libsaip.so")], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1].split("@")[0] for line in out.splitlines() if line.split()}
    exported = {s for s in exported if s.startswith("saip_")}
    declared = set(L._declared)
    assert exported - declared == set(), "exported but not in the ctypes table (an unmangled internal helper?)"
    assert declared - exported == set(), "declared but not exported (an entry lost in a unit?)"


def test_every_csrc_file_is_on_the_build_lists():
    from sai_primitives_amd import capi
    on_disk = lambda pat: {"csrc/" + os.path.basename(f) for f in glob.glob(os.path.join(PKG, "csrc", pat))}
    assert on_disk("*.cpp") | on_disk("*.hip") == set(capi.SOURCES)
    assert on_disk("*.h") <= set(capi.HEADERS), sorted(on_disk("*.h") - set(capi.HEADERS))
    assert len(set(capi.SOURCES)) == len(capi.SOURCES) and len(set(capi.HEADERS)) == len(capi.HEADERS)
    for rel in capi.SOURCES + capi.HEADERS:
        assert os.path.exists(os.path.join(PKG, rel)), rel
