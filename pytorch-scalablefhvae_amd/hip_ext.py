"""hip_ext.py -- what the satellite modules share around their launches ("Satellites").

A satellite is a csrc/*.hip file with its own header under include/, exported from libfhvae_hip.so but kept out of
include/fhvae_hip.h, and a Python module that holds the table of its entry points.  The launch itself goes through
hip_binding._call; this module is the rest:

  load             the library with a module's table bound
  rows_dense, pad_rows, padded_rows   the (N, D) f32 row operand: the one stride / alignment rule, the zero padding
  device_tensor    the "device tensor of this dtype / rank / shape" check with the module's noun in the message
  class_rows       the (N, C) f32 rows of per-frame class scores the trellis kernels take (ctc, falign, ctcbeam)
  host_ptr, groups, BatchPlan         a ragged batch: its (U + 1,) pointers on the host, the consecutive groups whose
                   workspace fits a byte limit, and the groups' rebased pointer rows on the device
  workspace        a grow-only byte buffer per owner and device
  status_word, check_status           the int32 device status word and its one read

Plain functions and one plain class; importing it needs neither a GPU nor torch.cuda.
"""
from __future__ import annotations

_bound = {}  # id(table) -> the library object the table was last bound on
_workspaces = {}  # (owner, device) -> uint8 device tensor


def load(signatures):
    """hip_binding.load_library() with the entry points of `signatures` (name -> (restype, argtypes)) bound.  A table is bound
    once per library object: a new library (hip_binding._lib replaced) gets it again."""
    import hip_binding as hb

    lib = hb.load_library()
    if _bound.get(id(signatures)) is not lib:
        for name, (res, args) in signatures.items():
            fn = getattr(lib, name)  # AttributeError if the .so lacks the symbol
            fn.restype, fn.argtypes = res, args
        _bound[id(signatures)] = lib
    return lib


def rows_dense(t, width):
    """Whether the kernels take the (N, width) f32 matrix as it is: unit column stride, a row stride that is a multiple of 4
    and at least `width`, a 16-byte aligned start."""
    return t.stride(1) == 1 and t.stride(0) >= width and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0


def pad_rows(t, multiple):
    """(N, D) -> rows of a width that is a multiple of `multiple`: zero-padded columns, or a dense copy of a view that is not
    rows_dense, or t itself."""
    import torch

    D = int(t.shape[1])
    if D % multiple:
        return torch.nn.functional.pad(t, (0, multiple - D % multiple))
    return t if rows_dense(t, D) else t.contiguous()


def padded_rows(op, name, t, noun, multiple, max_width, max_rows):
    """The (N, D) f32 rows of a call -> (pad_rows(t, multiple), D), after the checks: 2-D and not empty, on the device, float32,
    within the limits.  `noun` names the feature in the messages ("the probe")."""
    import torch

    if t is None or not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise RuntimeError("%s: %s must be a 2-D tensor with at least one row and one column" % (op, name))
    if not t.is_cuda:
        raise RuntimeError("%s: %s is a CPU tensor: %s runs on a MI355X only (no CPU fallback)" % (op, name, noun))
    if t.dtype != torch.float32:
        raise RuntimeError("%s: %s must be float32 (got %s)" % (op, name, t.dtype))
    D = int(t.shape[1])
    if D > max_width:
        raise RuntimeError("%s: %s has %d columns, %s kernels take at most %d" % (op, name, D, noun, max_width))
    if t.shape[0] > max_rows:
        raise RuntimeError("%s: %s has %d rows, %s kernels take at most %d" % (op, name, t.shape[0], noun, max_rows))
    return pad_rows(t, multiple), D


def device_tensor(op, name, t, noun, dtype=None, dim=None, shape=None, contiguous=False):
    """t if it is a device tensor of `dtype` (one, or a tuple of them), `dim` dimensions, `shape`, contiguous -- whichever are
    given; RuntimeError otherwise."""
    import torch

    if t is None or not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("%s: %s must be a device tensor: %s runs on a MI355X only (no CPU fallback)" % (op, name, noun))
    dtypes = () if dtype is None else (dtype if isinstance(dtype, tuple) else (dtype,))
    if ((dtypes and t.dtype not in dtypes) or (dim is not None and t.dim() != dim) or (shape is not None and tuple(t.shape) != tuple(shape))
            or (contiguous and not t.is_contiguous())):
        want = (["contiguous"] if contiguous else []) + (["%d-D" % dim] if dim is not None else []) + [" or ".join(str(d) for d in dtypes)]
        want += ["of shape %s" % (tuple(shape),)] if shape is not None else []
        raise RuntimeError("%s: %s must be %s (got %s %s)" % (op, name, " ".join(w for w in want if w), t.dtype, tuple(t.shape)))
    return t


def class_rows(op, logits, noun, max_classes):
    """(N, C) f32 device rows of per-frame class scores -> rows the kernels take as they are: unit column stride, a leading
    dimension that is a multiple of 4 and at least C, 16-byte aligned.  `noun` names the feature in the message."""
    import torch

    n_classes = int(logits.shape[1])
    if n_classes < 2 or n_classes > max_classes:
        raise RuntimeError("%s: %d classes, %s takes 2 to %d" % (op, n_classes, noun, max_classes))
    if logits.shape[0] and not rows_dense(logits, n_classes):
        logits = torch.nn.functional.pad(logits, (0, -n_classes % 4)) if n_classes % 4 else logits.contiguous()
    return logits


# ------------------------------------------------------------------------------------------------------------ ragged batches
def host_ptr(op, name, p):
    """A (U + 1,) pointer array as int64 numpy (a device tensor is copied: one sync), monotone from 0."""
    import numpy as np

    a = np.asarray(p.cpu() if hasattr(p, "cpu") else p)
    if a.ndim != 1 or a.shape[0] < 1 or a.dtype.kind not in "iu":
        raise RuntimeError("%s: %s must hold U + 1 integers" % (op, name))
    a = a.astype(np.int64)
    if a[0] != 0 or (np.diff(a) < 0).any():
        raise RuntimeError("%s: %s is not monotone from 0" % (op, name))
    return a


def groups(need_bytes, ws_limit):
    """Consecutive groups [(a, b)] of utterances whose summed workspace bytes fit ws_limit; an utterance larger than the limit
    gets a group of its own."""
    out, a, run = [], 0, 0
    for u, n in enumerate(need_bytes):
        if u > a and run + n > ws_limit:
            out.append((a, u))
            a, run = u, 0
        run += int(n)
    if len(need_bytes) > a:
        out.append((a, len(need_bytes)))
    return out


class BatchPlan:
    """The host side of a ragged batch, built once: the groups and their rebased pointer arrays on the device.

      utt, lab   the (U + 1,) int64 host pointers of host_ptr (lab is None for a batch without labels); U
      parts      [(a, b, ptrs)]: the utterances a .. b - 1 go in one call; ptrs is an int64 device tensor whose rows are
                 utt[a : b + 1] - utt[a], then (with labels) lab[a : b + 1] - lab[a], then the group's cumulative cells from 0
      ws_cells   the cells of the largest group

    need(utt, lab) gives the workspace cells per utterance, cell_bytes the bytes of one; ws_limit None puts all utterances
    into one group."""

    def __init__(self, op, utt_ptr, lab_ptr, device, need, cell_bytes, ws_limit):
        import numpy as np
        import torch

        self.utt = host_ptr(op, "utt_ptr", utt_ptr)
        self.lab = host_ptr(op, "lab_ptr", lab_ptr) if lab_ptr is not None else None
        if self.lab is not None and self.utt.shape != self.lab.shape:
            raise RuntimeError("%s: utt_ptr holds %d entries, lab_ptr %d" % (op, self.utt.shape[0], self.lab.shape[0]))
        self.U = int(self.utt.shape[0]) - 1
        cells = np.asarray(need(self.utt, self.lab), dtype=np.int64)
        self.parts = []
        self.ws_cells = 0
        for a, b in (groups(int(cell_bytes) * cells, int(ws_limit)) if ws_limit is not None else ([(0, self.U)] if self.U else [])):
            cell = np.concatenate([[0], np.cumsum(cells[a:b])]).astype(np.int64)
            rows = [p[a:b + 1] - p[a] for p in (self.utt, self.lab) if p is not None] + [cell]
            self.parts.append((a, b, torch.from_numpy(np.stack(rows)).to(device)))
            self.ws_cells = max(self.ws_cells, int(cell[-1]))


def workspace(owner, device, need):
    """`need` bytes on `device` for `owner`: the owner's buffer there if it is large enough, else a new one that replaces it."""
    import torch

    ws = _workspaces.get((owner, device))
    if ws is None or ws.numel() < need:
        ws = _workspaces[(owner, device)] = torch.empty(need, dtype=torch.uint8, device=device)
    return ws


def status_word(device):
    """A zeroed (1,) int32 status word on `device`."""
    import torch

    return torch.zeros(1, dtype=torch.int32, device=device)


def check_status(symbol, status, bits):
    """Reads the status word (one host sync) and raises on what the kernels refused: `bits` is [(bit, message)] in order."""
    st = int(status.item())
    if st:
        raise RuntimeError("%s: %s (status %d)" % (symbol, "; ".join(m for bit, m in bits if st & bit), st))
