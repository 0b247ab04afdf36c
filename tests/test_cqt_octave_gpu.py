"""Every instance and route of the constant-Q kernels on the MI355X (cases and reference: tests/cqt_cases.py; the same cases on the host simulator:
tests/test_cqt_octave_host.py).

* The fused octave kernel (csrc/lra_mixed.h: cqt_octave_body), all eight frame lengths in both precisions, driven through ``lra_cqt_octave_exec`` on device tensors
  into poisoned results: against the plain float64 reference at the per-row bar of cqt_cases (4 x the plain float32 computation's own error; x 2**-29 in float64),
  the row without entries exactly zero, nothing stored outside the octave's columns, a clip of the batch == that clip alone, the 8-byte sample loads == the scalar
  loads (a base address one element past alignment), and frames that move to another slot of their workgroup unchanged (constant padding, a shifted signal).
* ``librosa_amd.cqt`` / ``vqt`` calls whose plans reach every frame length, the merged launches included (ctx option cqt_merge 1 / 2 / 0, the Python loop), and the
  two-launch route (ones-window STFT + cqt_project_kernel) for all of them and for a frame length beyond the fused list: against cqt_oracle at the whole-transform bar.
* ``cqt_project_kernel`` alone against the float64 reference at the per-row bar.

Every test prints the figures it compares before it asserts.
"""
import numpy as np
import pytest

import cqt_cases as C
import librosa_amd as L
from librosa_amd import _arrays
from librosa_amd.core import constantq

pytestmark = pytest.mark.gpu


def _torch():
    import torch

    return torch


def _dev(a, misalign=False):
    """A device copy (the shared inputs are read-only); misalign: its base address one element past the allocation's alignment."""
    torch = _torch()
    t = torch.from_numpy(np.array(a)).cuda()
    if not misalign:
        return t
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % (2 * t.element_size()) == t.element_size() and view.is_contiguous()
    return view


def _poisoned(shape, dtype):
    torch = _torch()
    out = torch.empty(shape, dtype=torch.complex128 if np.dtype(dtype) == np.float64 else torch.complex64, device="cuda")
    torch.view_as_real(out).view(torch.uint8).fill_(0xFF)
    return out


def _still_poison(a):
    return bool(np.all(np.ascontiguousarray(a).view(np.uint8) == 0xFF))


TABLES = {}


def _tables(inst, c):
    key = (inst[0], np.dtype(inst[1]).str)
    if key not in TABLES:
        TABLES[key] = tuple(_dev(c[k]) for k in ("row_ptr", "col", "val"))
    return TABLES[key]


def dev_octave(inst, run, c, y=None, misalign=False):
    """``lra_cqt_octave_exec`` on device tensors the way core/constantq.py drives it, into a result that arrives full of 0xFF bytes; returns the host copy."""
    n_fft, dtype = inst
    y = _dev(c["y"] if y is None else y, misalign)
    rp, col, val = _tables(inst, c)
    sl = _dev(c["sqrt_len"]) if c["sqrt_len"] is not None else None
    out = _poisoned((y.shape[0], run["n_frames"], run["n_total"]), dtype)
    sess = _arrays.Session(y)
    try:
        sess.ctx.cqt_octave_exec(y.data_ptr(), y.shape[0], y.shape[1], y.shape[1], n_fft, run["hop"], run["pad_mode"], rp.data_ptr(), col.data_ptr(), val.data_ptr(),
                                 sl.data_ptr() if sl is not None else None, out.data_ptr(), run["n_frames"], run["n_total"], run["bin0"], run["row0"], run["n_rows"], np.dtype(dtype))
    finally:
        sess.close()
    return out.cpu().numpy()


# ---- the fused octave, directly ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inst", C.INSTANCES, ids=C.instance_id)
def test_octave_instance_is_reference(inst):
    worst = 0.0
    for run in C.family(inst):
        c = C.build(inst, run)
        got = dev_octave(inst, run, c)
        ratio, msg = C.compare(got, c, run)
        print(msg)
        worst = max(worst, ratio)
        assert ratio <= c["bar"], msg
        bin0, n_rows = run["bin0"], run["n_rows"]
        assert _still_poison(got[:, :, :bin0]) and _still_poison(got[:, :, bin0 + n_rows :]), (run["name"], "stored outside the octave's columns")
        if run["row0"] == 0:
            assert np.all(got[:, :, bin0] == 0), (run["name"], "the row without entries")
        for i in range(C.BATCH):
            alone = dev_octave(inst, run, c, y=c["y"][i : i + 1])
            assert np.array_equal(alone[0, :, bin0 : bin0 + n_rows], got[i, :, bin0 : bin0 + n_rows]), (run["name"], f"clip {i} alone differs from clip {i} of the batch")
        if run["hop"] % 2 == 0:
            shifted = dev_octave(inst, run, c, misalign=True)
            assert np.array_equal(shifted[:, :, bin0 : bin0 + n_rows], got[:, :, bin0 : bin0 + n_rows]), (run["name"], "scalar loads differ from 8-byte loads")
    print(f"instance {C.instance_id(inst)}: worst ratio {worst:.3g}")


@pytest.mark.parametrize("inst", C.INSTANCES, ids=C.instance_id)
def test_octave_frames_do_not_depend_on_their_slot(inst):
    """Constant padding: frame f of y[:, s * hop:] reads the samples of frame f + s of y once it starts at or after the cut, so the two are equal bit for bit; s = 3
    is a multiple of no frames-per-group above 1 that the kernel uses (8, 5, 2), so every such frame sits in another slot of its workgroup, and in another group."""
    s = 3
    runs = {r["name"]: r for r in C.family(inst)}
    for base in (runs["even-constant-scaled"], dict(runs["odd-reflect-scaled"], pad_mode="constant", name="odd-constant-scaled")):
        c = C.build(inst, runs["even-constant-scaled"] if base["hop"] % 2 == 0 else runs["odd-reflect-scaled"])   # (the signal, rows and scaling; the reference is not used)
        hop, bin0, n_rows = base["hop"], base["bin0"], base["n_rows"]
        whole = dev_octave(inst, base, c)
        cut = np.ascontiguousarray(c["y"][:, s * hop :])
        part = dev_octave(inst, dict(base, n_frames=base["n_frames"] - s), c, y=cut)
        first = -(-(inst[0] // 2) // hop)   # the first frame of the cut signal that reaches no sample before the cut
        assert first < base["n_frames"] - s - 2
        same = np.array_equal(part[:, first:, bin0 : bin0 + n_rows], whole[:, first + s :, bin0 : bin0 + n_rows])
        print(f"{C.instance_id(inst)} {base['name']}: frames {first}..{base['n_frames'] - s - 1} of the cut signal against frames {first + s}.. of the whole: {'equal' if same else 'DIFFERENT'}")
        assert same, base["name"]


# ---- the public API -----------------------------------------------------------------------------------------------------------------------------
def _cqt_close(Cq, ref):
    """tests/test_gpu_parity.py's bar for whole transforms."""
    tol = 1e-11 if Cq.dtype == np.complex128 else 2e-5
    return Cq.shape == ref.shape and Cq.dtype == ref.dtype and np.abs(Cq - ref).max() <= tol * np.abs(ref).max()


def _whole(name, fn, kw, y):
    return getattr(L, fn)(y, sr=C.SR, res_type="polyphase", **kw)


@pytest.mark.filterwarnings("ignore:n_fft=")
@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("name", C.WHOLE_IDS)
def test_whole_transform_every_route(name, dtype, monkeypatch):
    torch = _torch()
    _, fn, kw, plan = C.WHOLE[C.WHOLE_IDS.index(name)]
    ref = C.whole_oracle(name, dtype)
    y = _dev(C.whole_signal(dtype))
    fused_list = all(n in C.SIZES for n in plan)
    assert fused_list or not any(n in C.SIZES for n in plan)
    ctx = L.get_context(0)
    try:
        outs = {}
        for merge in (1, 2, 0):
            ctx.set_option("cqt_merge", merge)
            outs[f"cqt_merge={merge}"] = _whole(name, fn, kw, y)
    finally:
        ctx.set_option("cqt_merge", 1)
    monkeypatch.setattr(constantq, "NATIVE_RECURSION", False)
    outs["python loop"] = _whole(name, fn, kw, y)
    monkeypatch.setattr(constantq, "NATIVE_RECURSION", True)
    monkeypatch.setattr(constantq, "FUSED_OCTAVES", False)
    two = _whole(name, fn, kw, y)
    monkeypatch.setattr(constantq, "FUSED_OCTAVES", True)
    torch.cuda.synchronize()
    got = outs["cqt_merge=1"].cpu().numpy()
    err = np.abs(got - ref).max() / np.abs(ref).max()
    err_two = np.abs(two.cpu().numpy() - ref).max() / np.abs(ref).max()
    print(f"{name} {np.dtype(dtype).name}: plan {plan}, {'fused' if fused_list else 'two-launch'} {err:.3g}, two-launch route {err_two:.3g} of the peak")
    assert _cqt_close(got, ref), (name, err)
    for label, o in outs.items():
        assert torch.equal(o, outs["cqt_merge=1"]), (name, label)
    assert _cqt_close(two.cpu().numpy(), ref), (name, "two-launch route", err_two)
    if not fused_list:   # beyond the list: the two-launch route by itself
        assert torch.equal(two, outs["cqt_merge=1"]), name


# ---- the projection kernel, directly --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", C.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("n_fft", C.PROJECT_SIZES)
def test_project_kernel_is_reference(n_fft, dtype):
    c = C.build_project(n_fft, dtype)
    D, rp, col, val = (_dev(c[k]) for k in ("D", "row_ptr", "col", "val"))
    for case in c["cases"]:
        sl = _dev(case["sqrt_len"]) if case["sqrt_len"] is not None else None
        out = _poisoned((D.shape[0], case["n_frames"], case["n_total"]), dtype)
        sess = _arrays.Session(D)
        try:
            sess.ctx.cqt_project_exec(D.data_ptr(), out.data_ptr(), rp.data_ptr(), col.data_ptr(), val.data_ptr(), sl.data_ptr() if sl is not None else None, D.shape[0], D.shape[1], D.shape[2],
                                      case["n_frames"], case["n_total"], case["bin0"], case["row0"], case["n_rows"], np.dtype(dtype))
        finally:
            sess.close()
        got = out.cpu().numpy()
        ratio, msg = C.compare(got, case, case)
        print(msg)
        assert ratio <= case["bar"], msg
        bin0, n_rows = case["bin0"], case["n_rows"]
        assert _still_poison(got[:, :, :bin0]) and _still_poison(got[:, :, bin0 + n_rows :]), (case["name"], "stored outside the octave's columns")
        if case["row0"] == 0:
            assert np.all(got[:, :, bin0] == 0), (case["name"], "the row without entries")
