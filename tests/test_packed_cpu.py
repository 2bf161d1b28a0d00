"""Packed ragged output and float32 samples without a GPU: the float32 stores and the float32 form of the
output filter as a CPU program (tests/cpp/f32_pack_main.cpp: csrc/tree_core.h F32Pack and
output_filter_run_f32, csrc/afs_audio.h sample_to_f32) built with AddressSanitizer and
UndefinedBehaviorSanitizer and run directly; the header, the library and the binding name the new entry
points; afs_ragged_offsets; the refusals that need no context, and those the binding makes itself.  (The
library's own refusals need a context, so a GPU: tests/test_packed_gpu.py.)"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from areafunctionsynthesis_amd import _native
from areafunctionsynthesis_amd import synthesizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "areafunctionsynthesis_amd", "csrc")
ENTRY_POINTS = ("afs_synthesize_f32", "afs_synthesize_ragged_packed", "afs_ragged_offsets",
                "afs_session_synthesize_ragged_packed")
NF = np.array([7, 2, 5, 5, 3, 7, 2, 5, 5, 5, 5, 5, 5, 5, 5, 4, 5, 6, 6, 2, 3], dtype=np.int32)  # (tests/test_ragged_gpu.py)


def test_f32_pack_and_filter_form(tmp_path):
    """sample_to_f32 against the cast (+-0, denormals, ties, the range's edge, +-inf, NaN); every row
    alignment 0..3 and run length 0..24 against the casts, nothing written outside the run; the float32
    filter form against the cast of output_filter_run's doubles for n = 1..40 at every split, with and
    without the tone filter: bit-equal floats and state images."""
    exe = str(tmp_path / "f32_pack_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                           "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-ffp-contract=off", "-fno-strict-aliasing", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "f32_pack_main.cpp"), os.path.join(CSRC, "afs_tables.cpp"),
                           "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stdout + r.stderr[-3000:]
    assert r.stdout.strip() == "f32-ok"


def test_entry_points_declared_and_bound():
    with open(os.path.join(ROOT, "include", "afs.h"), encoding="utf-8") as fh:
        text = fh.read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _native.load()
    for name in ENTRY_POINTS:
        assert re.search(r"\bafs_status\s+" + name + r"\s*\(", header), name
        assert name in _native.EXPORTED
        assert hasattr(lib, name), name
        assert getattr(lib, name).restype is ctypes.c_int and getattr(lib, name).argtypes
    assert re.search(r"#define\s+AFS_ABI_VERSION\s+5\b", header)  # (an addition only)
    enum = header[header.index("typedef enum afs_sample_format"):header.index("} afs_sample_format;")]
    values = dict((n, int(v)) for n, v in re.findall(r"\b(AFS_SAMPLE_[A-Z0-9]+) = (\d+)", enum))
    assert values == {"AFS_SAMPLE_I16": _native.AFS_SAMPLE_I16, "AFS_SAMPLE_F32": _native.AFS_SAMPLE_F32}


@pytest.mark.parametrize("hop", [1, 37, 441])
def test_ragged_offsets(hop):
    off = synthesizer.ragged_offsets(NF, hop)
    lengths = (NF.astype(np.int64) - 1) * hop
    assert off.dtype == np.int64 and off.shape == (len(NF) + 1,)
    assert off[0] == 0 and np.array_equal(np.diff(off), lengths) and off[-1] == lengths.sum()
    assert np.array_equal(synthesizer.ragged_offsets([], hop), [0])
    assert np.array_equal(synthesizer.ragged_offsets([1, 3, 1], hop), [0, 0, 2 * hop, 2 * hop])


def test_ragged_offsets_do_not_wrap():
    """8 192 utterances of 2**20 frames at hop 441: the total is past 2**31 samples."""
    off = synthesizer.ragged_offsets(np.full(8192, 1 << 20, dtype=np.int32), 441)
    assert int(off[-1]) == 8192 * ((1 << 20) - 1) * 441 > 1 << 31


def test_tight_rows_start_at_every_alignment():
    """Hop 37 (odd) over the 21 lengths, as tests/test_packed_gpu.py packs them: tightly packed float32 rows
    start at every alignment mod 4.  For int16 mod 8 the rows in call order start at 7 of the 8 (the partial
    sums of NF - 1 never reach 5 mod 8, and an odd hop only permutes the residues); the same layout at a base
    one sample on -- the GPU test's odd device base -- reaches the eighth, as does the reversed layout."""
    off = synthesizer.ragged_offsets(NF, 37)[:-1]
    assert set(off % 4) == set(range(4))
    assert set(off % 8) == set(range(8)) - {1}
    assert set(off % 8) | set((off + 1) % 8) == set(range(8))
    rev = synthesizer.ragged_offsets(NF[::-1], 37)[:-1]
    assert set(off % 8) | set(rev % 8) == set(range(8))


def test_refusals_without_a_context():
    lib = _native.load()
    off = np.zeros(4, dtype=np.int64)
    nf = np.array([3, 2, 4], dtype=np.int32)
    vp = ctypes.c_void_p
    assert lib.afs_ragged_offsets(vp(nf.ctypes.data), 3, 5, vp(off.ctypes.data)) == 0 and list(off) == [0, 10, 15, 30]
    assert lib.afs_ragged_offsets(None, 3, 5, vp(off.ctypes.data)) == 1
    assert lib.afs_ragged_offsets(vp(nf.ctypes.data), 3, 5, None) == 1
    assert lib.afs_ragged_offsets(vp(nf.ctypes.data), -1, 5, vp(off.ctypes.data)) == 1
    assert lib.afs_ragged_offsets(vp(nf.ctypes.data), 3, 0, vp(off.ctypes.data)) == 1
    bad = np.array([3, 0, 4], dtype=np.int32)
    before = off.copy()
    assert lib.afs_ragged_offsets(vp(bad.ctypes.data), 3, 5, vp(off.ctypes.data)) == 1 and np.array_equal(off, before)
    with pytest.raises(_native.AfsError, match="invalid argument"):
        synthesizer.ragged_offsets([2, 0], 5)
    # (no context, no session: refused before anything is looked at)
    assert lib.afs_synthesize_f32(None, None, None, 1, 2, 5, None, 5, None, None) == 1
    assert lib.afs_synthesize_ragged_packed(None, None, 2, None, None, 1, 5, 0, None, None, None, None) == 1
    assert lib.afs_session_synthesize_ragged_packed(None, None, 2, None, 5, 0, None, None, None, None, None) == 1


def test_format_switches():
    """pcm and f32 together is an error; packed without either names the missing float64 form."""
    fmt = synthesizer._sample_format
    assert fmt(False, False) == (None, np.float64)
    assert fmt(True, False) == (_native.AFS_SAMPLE_I16, np.int16) and fmt(False, True, True) == (_native.AFS_SAMPLE_F32, np.float32)
    with pytest.raises(ValueError, match="pcm and f32"):
        fmt(True, True)
    with pytest.raises(ValueError, match="no packed float64 form"):
        fmt(False, False, True)


def test_packed_destination():
    """The binding's view of a packed destination: tight offsets and an array of the span when none is given;
    the caller's offsets as given; a wrong dtype, a 2-D array and a short array refused."""
    po = synthesizer._packed_out
    out, addr, off, own = po(None, None, [10, None, 0, 7], np.float32)
    assert out.dtype == np.float32 and out.shape == (17,) and list(off) == [0, 10, 10, 10, 17] and own is None and addr
    mine = np.array([40, 3, 3, 20], dtype=np.int64)
    out, addr, off, own = po(None, mine, [10, None, 0, 7], np.int16)
    assert out.dtype == np.int16 and out.shape == (50,) and off is not None and list(own) == list(mine)
    with pytest.raises(ValueError, match="contiguous int16"):
        po(np.zeros(50, dtype=np.float32), mine, [10, None, 0, 7], np.int16)
    with pytest.raises(ValueError, match="1-D"):
        po(np.zeros((5, 10), dtype=np.int16), mine, [10, None, 0, 7], np.int16)
    with pytest.raises(ValueError, match="50 samples"):
        po(np.zeros(49, dtype=np.int16), mine, [10, None, 0, 7], np.int16)
    with pytest.raises(ValueError, match="one row start"):
        po(None, mine[:2], [10, None, 0, 7], np.int16)
