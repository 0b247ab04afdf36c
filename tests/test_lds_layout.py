"""LDS layouts of the two FFT exchanges of the one-wave n_fft = 2048 float32 cores (librosa_amd/csrc/lra_fft.h, "exchange addresses").

tests/lds_layout_check.cpp evaluates the address functions the kernels call for all 64 lanes and every compile-time index and counts LDS-array
cycles per wave instruction by gfx950's lane groups and bank rules (scripts/lds_model.py, GROUPS).  Asserted here: both exchanges of the
16-8-8 core and exchange 1 of the 16-16-4 core have no conflict cycle (the padded layout phys() had 32 + 32: every ds_read_b64 of a 32-lane
group straddled one pad unit), every unit stored is read back and nothing else is read, and the layouts stay inside FftCfg::FRAME_BYTES."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "lds_layout_check.cpp")


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lds_layout") / "lds_layout_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-w", SRC, "-o", exe])
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert "error=" not in out, out
    parsed = []
    for line in out.strip().splitlines():
        kv = dict(f.split("=", 1) for f in line.split())
        parsed.append({k: (v if k == "plan" else int(v)) for k, v in kv.items()})
    print(out)
    return {(r["plan"], r["exchange"]): r for r in parsed}


def test_exchanges_present(rows):
    assert set(rows) == {("16-8-8", 1), ("16-8-8", 2), ("16-16-4", 1), ("16-8-8/mel", 1), ("16-8-8/mel", 2)}
    # exchange 1 transposed on both plans, exchange 2 unpadded on 16-8-8
    assert all(r["layout"] == (1 if ex == 1 else 2) for (_, ex), r in rows.items())


@pytest.mark.parametrize("key", [("16-8-8", 1), ("16-8-8", 2), ("16-16-4", 1), ("16-8-8/mel", 1), ("16-8-8/mel", 2)])
def test_exchange_conflict_free_and_closed(rows, key):
    r = rows[key]
    assert r["write_insts"] == 16 and r["read_insts"] == 16
    assert r["write_conflicts"] == 0 and r["read_conflicts"] == 0, r
    # conflict-free cost: four 16-lane groups per ds_write_b64, two 32-lane groups per ds_read_b64
    assert r["write_cycles"] == 16 * 4 and r["read_cycles"] == 16 * 2, r
    assert r["sets_equal"] == 1 and r["units_written"] == 1024 and r["units_read"] == 1024, r
    assert 0 < r["footprint_bytes"] <= r["frame_bytes"], r
