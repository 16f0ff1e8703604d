"""CPU: the host side of the chained dense-block launch -- the schedule header's constexpr checks (the 40-step walk, the
re-entry at a block boundary, the buffer rotation) compile with the host compiler on that file alone, and the per-block table
(nesr_rdb_chain_table, host only) holds the rotation of the three trunk buffers and each block's five weight and bias
addresses as the forward's dense-block loop uses them."""
import ctypes
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "neural_enhanced_super_resolution_amd", "csrc")


def test_schedule_header_checks_compile_on_the_host():
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or shutil.which("hipcc")
    assert cxx is not None, "no host C++ compiler (the library itself needs one to build)"
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-x", "c++", os.path.join(CSRC, "rdb_f16x2_schedule.h")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # the same file from a translation unit: what the kernel and the host code take from it
    src = ('#include "rdb_f16x2_schedule.h"\n'
           'using namespace nesr::rdbs;\n'
           'static_assert(chain_reentry_ok() && chain_war_ok(), "");\n'
           'static_assert(CHAIN_BARS == nesr::RDB_STEPS + 2 && REENTRY_TAIL_FIRST == IN_LEAD - 1 && REENTRY_TAIL_0 < REENTRY_TAIL_FIRST, "");\n'
           'static_assert(rdb_cur_buf(2) == 2 && rdb_out_buf(2) == 0 && rdb_res2_buf(2) == 0 && rdb_res2_buf(1) < 0, "");\n')
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-x", "c++", "-"], capture_output=True, text=True, cwd=CSRC, input=src)
    assert r.returncode == 0, r.stderr
    # ... and the asserts are live: a stagger the walk does not cover is refused
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-DNESR_RDB_LAG=4", "-x", "c++", os.path.join(CSRC, "rdb_f16x2_schedule.h")],
                       capture_output=True, text=True)
    assert r.returncode != 0


def test_block_table_rotation_and_pointers():
    from neural_enhanced_super_resolution_amd import _lib
    lib = _lib.load()
    nb = 2
    nl = 1 + 15 * nb
    bufs = (ctypes.c_uint64 * 3)(0xA000, 0xB000, 0xC000)
    w = (ctypes.c_uint64 * nl)(*[0x100000 + 0x100 * i for i in range(nl)])
    b = (ctypes.c_uint64 * nl)(*[0x200000 + 0x10 * i for i in range(nl)])
    table = (ctypes.c_uint64 * (13 * 3 * nb))()
    assert lib.nesr_rdb_chain_table(nb, bufs, w, b, table) == 0
    for i in range(3 * nb):
        rrdb, r = divmod(i, 3)
        e = list(table[13 * i:13 * i + 13])
        # the dense-block loop: block r of an RRDB runs in buffer r, conv5 lands in the next buffer, the third block's in the
        # first in place, with the RRDB's input (that buffer) as second residual
        assert e[0] == bufs[r]
        assert e[1] == (bufs[r + 1] if r < 2 else bufs[0])
        assert e[2] == (0 if r < 2 else bufs[0])
        first = 1 + (rrdb * 3 + r) * 5
        assert e[3:8] == [w[first + k] for k in range(5)]
        assert e[8:13] == [b[first + k] for k in range(5)]
    assert lib.nesr_rdb_chain_table(0, bufs, w, b, table) == -1
    assert lib.nesr_rdb_chain_table(nb, None, w, b, table) == -1
