"""hip_ext without a GPU: a table is bound once per library object and again on a new one, a missing symbol raises, the one
dense-row rule on the views it must tell apart, the zero padding at the widths around both multiples, the grow-only workspaces
per owner, the refusals of a CPU tensor, and the status messages as abx, units, qbe and kaldi_post have always worded them."""
import ctypes as C

import pytest
import torch

import hip_ext


class _Fn:
    restype = argtypes = None


class _Lib:
    """Stands for a CDLL: an attribute per symbol; counts the getattr calls of a binding."""

    def __init__(self, names):
        self.fns = {n: _Fn() for n in names}
        self.asked = 0

    def __getattr__(self, name):
        if name not in self.fns:
            raise AttributeError(name)
        self.asked += 1
        return self.fns[name]


TABLE = {"fhvae_x_ws_bytes": (C.c_int64, [C.c_int64]), "fhvae_x_run": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p])}


def test_load_binds_once_per_library_object(monkeypatch):
    import hip_binding as hb

    a, b = _Lib(TABLE), _Lib(TABLE)
    monkeypatch.setattr(hb, "_lib", a)
    assert hip_ext.load(TABLE) is a and a.asked == 2
    assert a.fns["fhvae_x_run"].restype is C.c_int and a.fns["fhvae_x_run"].argtypes == [C.c_void_p, C.c_int64, C.c_void_p]
    assert a.fns["fhvae_x_ws_bytes"].restype is C.c_int64
    assert hip_ext.load(TABLE) is a and a.asked == 2  # (bound already: nothing is looked up again)
    monkeypatch.setattr(hb, "_lib", b)  # the library replaced, as tests/test_binding_calls_cpu.py does with its stub
    assert hip_ext.load(TABLE) is b and b.asked == 2 and b.fns["fhvae_x_run"].argtypes == TABLE["fhvae_x_run"][1]
    other = dict(TABLE)  # another module's table on the same library is bound on its own
    assert hip_ext.load(other) is b and b.asked == 4


def test_a_missing_symbol_raises(monkeypatch):
    import hip_binding as hb

    monkeypatch.setattr(hb, "_lib", _Lib(["fhvae_x_ws_bytes"]))
    with pytest.raises(AttributeError, match="fhvae_x_run"):
        hip_ext.load(TABLE)
    with pytest.raises(AttributeError):  # (and is not remembered as bound)
        hip_ext.load(TABLE)


def _base(rows, cols):
    """A (rows, cols) f32 matrix whose first element lies on a 16-byte boundary."""
    flat = torch.arange(1, rows * cols + 5, dtype=torch.float32)
    return flat[(-flat.data_ptr() % 16) // 4:][:rows * cols].view(rows, cols)


def test_rows_dense():
    m = _base(6, 24)
    assert m.data_ptr() % 16 == 0
    assert hip_ext.rows_dense(m, 24)  # contiguous
    assert hip_ext.rows_dense(m[:, :16], 16) and m[:, :16].stride(0) == 24  # a column slice, row stride 24 = 6 * 4
    assert hip_ext.rows_dense(m[:, 4:20], 16)  # (starting 16 bytes in)
    odd = _base(6, 22)[:, :16]
    assert odd.stride(0) == 22 and not hip_ext.rows_dense(odd, 16)  # a row stride that is no multiple of 4
    assert not hip_ext.rows_dense(_base(16, 6).t(), 16)  # transposed: the column stride is not 1
    assert not hip_ext.rows_dense(m[:, 1:17], 16)  # starts 4 bytes off a 16-byte boundary
    assert not hip_ext.rows_dense(m[:, :16], 32)  # rows narrower than the width asked for
    assert not hip_ext.rows_dense(m[:1].expand(6, 24), 24)  # one row repeated: row stride 0


@pytest.mark.parametrize("multiple,width", [(16, 1), (16, 15), (16, 16), (16, 17), (8, 7), (8, 8), (8, 9)])
def test_pad_rows(multiple, width):
    x = _base(5, width)
    out = hip_ext.pad_rows(x, multiple)
    W = -(-width // multiple) * multiple
    assert tuple(out.shape) == (5, W) and out.dtype == torch.float32
    assert torch.equal(out[:, :width], x) and not out[:, width:].any()  # the padding columns are exactly 0
    assert hip_ext.rows_dense(out, W)
    if width % multiple == 0:
        assert out is x  # dense already: taken as it is, no copy
        view = _base(5, width + 3)[:, :width]  # a view the kernels cannot take is copied, its values kept
        got = hip_ext.pad_rows(view, multiple)
        assert got is not view and got.is_contiguous() and torch.equal(got, view)


@pytest.mark.parametrize("multiple,width", [(16, 1), (16, 15), (16, 16), (16, 17), (8, 7), (8, 8), (8, 9)])
def test_padded_rows_stops_a_cpu_tensor_at_the_device_check(multiple, width):
    """padded_rows is its checks, then (pad_rows(t, multiple), D): a CPU tensor gets as far as the device check, what lies
    behind it is pad_rows above (tests/test_probe_gpu.py and tests/test_gmm_gpu.py run the whole on the device)."""
    x = torch.ones(3, width)
    with pytest.raises(RuntimeError, match=r"op: x is a CPU tensor: the probe runs on a MI355X only \(no CPU fallback\)"):
        hip_ext.padded_rows("op", "x", x, "the probe", multiple, 128, 1 << 30)


def test_padded_rows_and_device_tensor_refuse():
    for bad in (None, torch.zeros(3), torch.zeros(0, 4), torch.zeros(4, 0), [[1.0]]):
        with pytest.raises(RuntimeError, match="op: x must be a 2-D tensor with at least one row and one column"):
            hip_ext.padded_rows("op", "x", bad, "the mixture", 8, 64, 1 << 30)
    for bad in (None, torch.zeros(3), [1.0]):
        with pytest.raises(RuntimeError, match=r"op: y must be a device tensor: the mixture runs on a MI355X only \(no CPU fallback\)"):
            hip_ext.device_tensor("op", "y", bad, "the mixture", torch.float32, shape=(3,))


def test_groups_by_bytes():
    # (the cases ctc.groups was held to, its needs of 5, 50 .. float64 cells given in bytes)
    assert hip_ext.groups([40, 40, 40], 80) == [(0, 2), (2, 3)]
    assert hip_ext.groups([40, 400, 40, 0], 80) == [(0, 1), (1, 2), (2, 4)]
    assert hip_ext.groups([], 80) == [] and hip_ext.groups([8, 8], 1 << 30) == [(0, 2)]


def test_batch_plan_rebases_the_groups_and_counts_cells():
    import numpy as np

    def need(utt, lab):
        return np.diff(utt) * (2 * np.diff(lab) + 1)

    utt, lab = [0, 5, 5, 8, 9], torch.tensor([0, 2, 2, 3, 3])
    plan = hip_ext.BatchPlan("op", utt, lab, "cpu", need, 8, 8 * 25)
    assert plan.U == 4 and plan.utt.tolist() == utt and plan.lab.tolist() == [0, 2, 2, 3, 3] and plan.ws_cells == 25
    assert [(a, b) for a, b, _ in plan.parts] == [(0, 2), (2, 4)]
    assert plan.parts[0][2].tolist() == [[0, 5, 5], [0, 2, 2], [0, 25, 25]] and plan.parts[0][2].dtype == torch.int64
    assert plan.parts[1][2].tolist() == [[0, 3, 4], [0, 1, 1], [0, 9, 10]]
    one = hip_ext.BatchPlan("op", utt, lab, "cpu", need, 8, None)  # no limit: one group
    assert [(a, b) for a, b, _ in one.parts] == [(0, 4)] and one.ws_cells == 35
    bare = hip_ext.BatchPlan("op", utt, None, "cpu", lambda utt, lab: np.diff(utt), 16, 1 << 30)  # no labels: two rows
    assert bare.lab is None and bare.parts[0][2].tolist() == [[0, 5, 5, 8, 9], [0, 5, 5, 8, 9]] and bare.ws_cells == 9
    assert hip_ext.BatchPlan("op", [0], [0], "cpu", need, 8, 80).parts == []
    with pytest.raises(RuntimeError, match="op: utt_ptr holds 5 entries, lab_ptr 4"):
        hip_ext.BatchPlan("op", utt, [0, 2, 2, 3], "cpu", need, 8, 80)
    with pytest.raises(RuntimeError, match="op: utt_ptr is not monotone from 0"):
        hip_ext.BatchPlan("op", [0, 5, 4], [0, 1, 1], "cpu", need, 8, 80)
    with pytest.raises(RuntimeError, match="op: lab_ptr must hold U \\+ 1 integers"):
        hip_ext.BatchPlan("op", utt, np.zeros(5), "cpu", need, 8, 80)


def test_class_rows_names_the_feature():
    with pytest.raises(RuntimeError, match="op: 129 classes, forced alignment takes 2 to 128"):
        hip_ext.class_rows("op", torch.zeros(3, 129), "forced alignment", 128)
    with pytest.raises(RuntimeError, match="op: 1 classes, the CTC kernel takes 2 to 128"):
        hip_ext.class_rows("op", torch.zeros(3, 1), "the CTC kernel", 128)
    x = torch.zeros(5, 8)
    assert hip_ext.class_rows("op", x, "the CTC kernel", 128) is x  # dense rows are taken as they are
    y = hip_ext.class_rows("op", torch.ones(5, 6), "the CTC kernel", 128)
    assert tuple(y.shape) == (5, 8) and y.stride(0) == 8 and bool((y[:, 6:] == 0).all()) and bool((y[:, :6] == 1).all())


def test_workspace_grows_only_and_owners_do_not_share():
    a = hip_ext.workspace("test-owner-a", "cpu", 1024)
    assert a.dtype == torch.uint8 and a.numel() == 1024 and a.device.type == "cpu"
    assert hip_ext.workspace("test-owner-a", "cpu", 256) is a  # a smaller need: the same buffer
    assert hip_ext.workspace("test-owner-a", "cpu", 1024) is a
    b = hip_ext.workspace("test-owner-b", "cpu", 512)
    assert b is not a and b.numel() == 512 and b.data_ptr() != a.data_ptr()  # another owner: its own buffer
    big = hip_ext.workspace("test-owner-a", "cpu", 4096)
    assert big is not a and big.numel() == 4096  # a larger need replaces it
    assert hip_ext.workspace("test-owner-a", "cpu", 1024) is big and hip_ext.workspace("test-owner-b", "cpu", 512) is b


def test_status_word_and_the_messages():
    import abx
    import kaldi_post
    import qbe
    import units

    word = hip_ext.status_word("cpu")
    assert word.dtype == torch.int32 and tuple(word.shape) == (1,) and int(word) == 0
    abx.check_status(word), units.check_status(word)  # no bit: nothing is raised

    def message(check, st):
        with pytest.raises(RuntimeError) as e:
            check(torch.full((1,), st, dtype=torch.int32))
        return str(e.value)

    # the texts as abx, units and qbe raised them when each had its own copy of the check, verbatim
    assert message(abx.check_status, 1) == "fhvae_abx_dtw: a token lies outside the features or is longer than 64 frames (status 1)"
    assert message(abx.check_status, 2) == "fhvae_abx_dtw: grp_ptr / out_ptr / pair_ptr are inconsistent (status 2)"
    assert message(abx.check_status, 3) == ("fhvae_abx_dtw: a token lies outside the features or is longer than 64 frames; "
                                            "grp_ptr / out_ptr / pair_ptr are inconsistent (status 3)")
    assert message(units.check_status, 1) == "fhvae_km_update: cl_ptr is not monotone from 0 to N (a label outside [0, K)?) (status 1)"
    assert message(units.check_status, 2) == "fhvae_km_update: a perm entry lies outside [0, N) (status 2)"
    assert message(units.check_status, 3) == ("fhvae_km_update: cl_ptr is not monotone from 0 to N (a label outside [0, K)?); "
                                              "a perm entry lies outside [0, N) (status 3)")
    assert message(qbe.check_status, 3) == ("fhvae_qbe_sdtw: a query lies outside the features or is longer than its bound (at most 64 frames); "
                                            "utt_ptr is not monotone from 0 to the number of frames (status 3)")
    # kaldi_post words its one bit as features.py words its batches' status errors, and keeps that
    assert message(kaldi_post._check_status, 1) == "fhvae_kaldi_add_deltas / fhvae_kaldi_cmvn_sliding: status 1 (inconsistent frame_ptr)"
    kaldi_post._check_status(word)
