"""Loader for the in-tree HIP kernel library ``wellflow/_C.so``.

There is no fallback: GPU code paths call :func:`lib` and get an ImportError with the
build instruction when the extension is missing (the CPU oracle paths never touch it).
"""
from __future__ import annotations

import importlib
import os

_LIB = None


def lib():
    """Return the loaded ``wellflow._C`` module (raises if it was not built)."""
    global _LIB
    if _LIB is None:
        import torch  # noqa: F401  (loads libtorch / libamdhip64 first)

        try:
            _LIB = importlib.import_module("wellflow._C")
        except ImportError as e:  # pragma: no cover - depends on the build
            here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
            raise ImportError(
                f"wellflow native extension not built ({e}). Run `python -m wellflow._build` "
                f"(expects {os.path.join(here, '_C.so')})."
            ) from e
    return _LIB


def available() -> bool:
    try:
        lib()
        return True
    except ImportError:
        return False


ASSEMBLE_MAX_F = 512  # csrc/binding.cpp kAssembleMaxF: wider tables are assembled on the host


def assemble_features(codes, cont, cat_off, cat_size, mean, std, n_features: int, out_dtype, device, out=None):
    """Feature rows built on the device from raw columns (csrc/features.hip).

    ``codes`` int32 [C][N] and ``cont`` float32 [Q][N] (numpy or tensors; uploaded as they are —
    no widened [N][F] matrix crosses the bus), ``cat_off`` / ``cat_size`` [C] and ``mean`` /
    ``std`` [Q] from :meth:`FeaturePipeline.block_spec` / :meth:`~FeaturePipeline.scale`.
    ``out_dtype`` bf16 -> [N][round_up(F, 8)], the MLP input format; float32 -> [N][F], the LSTM
    row table (``out``: write into this tensor). One upload and one assembly of
    :class:`ResidentColumns`, which checks the block spec on the host before anything is launched;
    an empty table gives an empty result without a launch."""
    import torch

    res = ResidentColumns(codes, cont, cat_off, cat_size, mean, std, n_features, device)
    if res.N < 1:
        return torch.zeros((0, res.out_width(out_dtype)), dtype=out_dtype, device=res.device)
    return res.assemble(out_dtype, out=out)


class ResidentColumns:
    """A table's raw columns and its pipeline's block spec, checked on the host and uploaded ONCE:
    what the passes of a permutation-importance run (wellflow/importance.py) assemble from, over
    and over, without a further host check or H2D copy."""

    def __init__(self, codes, cont, cat_off, cat_size, mean, std, n_features: int, device):
        import numpy as np
        import torch

        self.device = dev = torch.device(device)
        self.F = F = int(n_features)
        off = np.asarray(cat_off, dtype=np.int64).reshape(-1)
        size = np.asarray(cat_size, dtype=np.int64).reshape(-1)
        codes, cont = torch.as_tensor(codes), torch.as_tensor(cont)
        self.C = C = codes.shape[0] if codes.dim() == 2 else 0
        self.Q = Q = cont.shape[0] if cont.dim() == 2 else 0
        self.N = codes.shape[1] if C else (cont.shape[1] if Q else 0)
        if len(off) != C or len(size) != C:
            raise ValueError(f"assemble_features: {C} code columns but {len(off)} offsets / {len(size)} sizes")
        if C and ((size < 0).any() or (off != np.cumsum(size) - size).any()):
            raise ValueError("assemble_features: one-hot blocks must be back to back from column 0")
        if int(size.sum()) + Q != F:
            raise ValueError(f"assemble_features: one-hot width {int(size.sum())} + {Q} continuous != F = {F}")
        if Q and (cont.shape[1] != self.N or len(mean) != Q or len(std) != Q):
            raise ValueError("assemble_features: cont / mean / std shapes disagree")
        if self.N >= 2 ** 31:
            raise ValueError(f"assemble_features: an int32 permutation cannot index {self.N} rows")
        i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32)).to(dev)  # noqa: E731
        f32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dev)  # noqa: E731
        self.codes = codes.to(dev, torch.int32).contiguous() if C else None
        self.cont = cont.to(dev, torch.float32).contiguous() if Q else None
        self.off, self.size = (i32(off), i32(size)) if C else (None, None)
        self.mean, self.std = (f32(mean), f32(std)) if Q else (None, None)

    def out_width(self, out_dtype) -> int:
        import torch

        return (self.F + 7) // 8 * 8 if out_dtype == torch.bfloat16 else self.F

    def assemble(self, out_dtype, rows=None, perm=None, perm_col: int = -1, out=None, const_col: int = -1,
                 const_value=None, col_set=None, perm_values=None):
        """Feature rows ``rows = (a, b)`` (default: all) of the resident table, as
        :func:`assemble_features` builds them. With ``perm`` (int32 device vector of ``b - a``
        indices into ALL N rows) source column ``perm_col`` — in the kernel's source order, the C
        categorical columns first, then the Q continuous ones — is read through it: output row r
        takes that column's value of row ``perm[r]`` (the kernel clamps the index into the
        column). With ``const_value`` (a contiguous one-element tensor on the table's device: an
        int32 label code for a categorical source, a float32 raw value for a continuous one)
        source column ``const_col`` is that constant in every output row; it goes through the
        kernel's own block test / standardisation, so the unknown index ``len(labels)`` gives the
        all-zero block. One column is permuted or constant, not both.
        With ``col_set`` (a row of :func:`column_masks`: int32 [ceil((C + Q) / 32)] on the table's
        device) EVERY source column of the set is read through ``perm`` (needed; ``perm_col`` stays
        -1): the set launch of the kernel. Not combined with ``perm_col`` or a constant.
        With ``perm_values`` (a contiguous float32 vector over ALL N rows on the table's device;
        together with ``perm`` and a CONTINUOUS ``perm_col``) the permuted column is read from
        that vector instead of the table: output row r takes ``perm_values[perm[r]]`` through the
        kernel's own standardisation, so with the identity ``perm[a:b]`` the column has one
        value per row. Not combined with ``col_set`` or a constant.
        Everything is refused here, on the host, before a launch; nothing is uploaded."""
        import torch

        a, b = (0, self.N) if rows is None else (int(rows[0]), int(rows[1]))
        if not 0 <= a < b <= self.N:
            raise ValueError(f"assemble_features: rows [{a}, {b}) outside the table's {self.N} rows")
        perm_col = int(perm_col)
        if perm_values is not None:
            if col_set is not None:
                raise ValueError("assemble_features: per-row values (perm_values) are not combined with a set of "
                                 "permuted columns (col_set)")
            if const_value is not None or int(const_col) >= 0:
                raise ValueError("assemble_features: per-row values (perm_values) are not combined with a constant column")
            if perm is None or perm_col < 0:
                raise ValueError("assemble_features: perm_values goes together with perm and perm_col")
            if not self.C <= perm_col < self.C + self.Q:
                raise ValueError(f"assemble_features: perm_values needs a continuous perm_col "
                                 f"([{self.C}, {self.C + self.Q})), got {perm_col}"
                                 f"{' (a categorical column)' if 0 <= perm_col < self.C else ''}")
            if not isinstance(perm_values, torch.Tensor) or perm_values.device != self.device:
                raise ValueError(f"assemble_features: perm_values must be a tensor on {self.device}")
            if perm_values.dtype != torch.float32:
                raise TypeError(f"assemble_features: perm_values must be float32, got {perm_values.dtype}")
            if perm_values.dim() != 1 or perm_values.numel() != self.N or not perm_values.is_contiguous():
                raise ValueError(f"assemble_features: perm_values holds {tuple(perm_values.shape)} values for the "
                                 f"table's {self.N} rows (a contiguous vector)")
        if col_set is not None:
            if perm_col >= 0:
                raise ValueError("assemble_features: a set of permuted columns (col_set) or ONE perm_col, not both")
            if const_value is not None or int(const_col) >= 0:
                raise ValueError("assemble_features: a set of permuted columns (col_set) is not combined with a "
                                 "constant column")
            if perm is None:
                raise ValueError("assemble_features: a set of permuted columns (col_set) needs perm")
            words = (self.C + self.Q + 31) // 32
            if not isinstance(col_set, torch.Tensor) or col_set.device != self.device:
                raise ValueError(f"assemble_features: col_set must be a tensor on {self.device}")
            if col_set.dtype != torch.int32:
                raise TypeError(f"assemble_features: col_set must be int32 (the mask's 32-bit words), got {col_set.dtype}")
            if col_set.dim() != 1 or col_set.numel() != words or not col_set.is_contiguous():
                raise ValueError(f"assemble_features: col_set holds {tuple(col_set.shape)} words for "
                                 f"{self.C + self.Q} source columns (need {words})")
        elif (perm is None) != (perm_col < 0):
            raise ValueError("assemble_features: perm and perm_col go together")
        if perm is not None:
            if col_set is None and not 0 <= perm_col < self.C + self.Q:
                raise ValueError(f"assemble_features: perm_col {perm_col} outside [0, {self.C + self.Q})")
            if not isinstance(perm, torch.Tensor) or perm.device != self.device:
                raise ValueError(f"assemble_features: perm must be a tensor on {self.device}")
            if perm.dtype != torch.int32:
                raise TypeError(f"assemble_features: perm must be int32, got {perm.dtype}")
            if perm.dim() != 1 or perm.numel() != b - a or not perm.is_contiguous():
                raise ValueError(f"assemble_features: perm holds {tuple(perm.shape)} indices for {b - a} rows")
        const_col = int(const_col)
        if (const_value is None) != (const_col < 0):
            raise ValueError("assemble_features: const_col and const_value go together")
        if const_value is not None:
            if perm is not None:
                raise ValueError("assemble_features: one source column is permuted or constant, not both "
                                 "(perm and const_col)")
            if not 0 <= const_col < self.C + self.Q:
                raise ValueError(f"assemble_features: const_col {const_col} outside [0, {self.C + self.Q})")
            if not isinstance(const_value, torch.Tensor) or const_value.device != self.device:
                raise ValueError(f"assemble_features: const_value must be a tensor on {self.device}")
            want = torch.int32 if const_col < self.C else torch.float32
            if const_value.dtype != want:
                raise TypeError(f"assemble_features: const_value must be {want} for a "
                                f"{'categorical' if const_col < self.C else 'continuous'} column, got {const_value.dtype}")
            if const_value.numel() != 1 or not const_value.is_contiguous():
                raise ValueError(f"assemble_features: const_value must be one contiguous element, got "
                                 f"{tuple(const_value.shape)}")
        ld = self.out_width(out_dtype)
        if out is None:
            out = torch.empty((b - a, ld), dtype=out_dtype, device=self.device)
        elif out.shape != (b - a, ld) or out.dtype != out_dtype or out.device != self.device:
            raise ValueError(f"assemble_features: out must be {out_dtype} [{b - a}][{ld}] on {self.device}")
        if col_set is not None:
            lib().assemble_features(self.codes, self.cont, self.off, self.size, self.mean, self.std, a, b - a, self.F,
                                    out, -1, perm, set_mask=col_set)
            return out
        if perm_values is not None:
            lib().assemble_features(self.codes, self.cont, self.off, self.size, self.mean, self.std, a, b - a, self.F,
                                    out, perm_col, perm, perm_values=perm_values)
            return out
        lib().assemble_features(self.codes, self.cont, self.off, self.size, self.mean, self.std, a, b - a, self.F, out,
                                perm_col if perm is not None else -1, perm, const_col if const_value is not None else -1,
                                const_value)
        return out


def column_masks(sets, n_sources: int, device=None):
    """The bitmasks of source-column sets for :meth:`ResidentColumns.assemble` (``col_set``):
    int32 ``[len(sets)][ceil(n_sources / 32)]``, the bit pattern of 32-bit words in which bit
    ``s & 31`` of word ``s >> 5`` is source column ``s``. A job builds the masks of all its passes
    in one call (one upload when ``device`` is given) and a pass points at its row."""
    import numpy as np
    import torch

    S = int(n_sources)
    if S < 1:
        raise ValueError(f"column_masks: {S} source columns")
    m = np.zeros((len(sets), (S + 31) // 32), np.uint32)
    for i, cols in enumerate(sets):
        for c in cols:
            c = int(c)
            if not 0 <= c < S:
                raise ValueError(f"column_masks: source column {c} outside [0, {S})")
            m[i, c >> 5] |= np.uint32(1) << np.uint32(c & 31)
    t = torch.from_numpy(m.view(np.int32))
    return t if device is None else t.to(device)


def err_sums(pred, y, y_scale: float, y_shift: float, out, slot: int, scratch):
    """``out[slot] = {sum d^2, sum |d|}``, ``d = pred * y_scale + y_shift - y`` in fp64
    (csrc/score.hip): fp32 device vectors ``pred`` / ``y`` of one length, ``out`` fp64 [S][2],
    ``scratch`` from :func:`err_sums_scratch`. Stream-ordered; nothing comes back to the host."""
    import torch

    if pred.dtype != torch.float32 or y.dtype != torch.float32:
        raise TypeError(f"err_sums: pred / y must be float32, got {pred.dtype} / {y.dtype}")
    if pred.dim() != 1 or pred.shape != y.shape or pred.numel() < 1:
        raise ValueError(f"err_sums: pred {tuple(pred.shape)} and y {tuple(y.shape)} must be equal, non-empty vectors")
    if out.dtype != torch.float64 or out.dim() != 2 or out.shape[1] != 2 or not 0 <= int(slot) < out.shape[0]:
        raise ValueError(f"err_sums: out must be float64 [S][2] with slot {slot} inside it")
    lib().err_sums(pred, y, float(y_scale), float(y_shift), out, int(slot), scratch)


def attr_step(p_cur, p_prev, y_scale: float, y_shift: float, acc, sq, row: int, start: bool = False):
    """One step of a sampling Shapley run (csrc/score.hip): in row ``row`` of the fp64 tables
    ``acc`` / ``sq`` ``[K + 1][M]``, ``d = (p_cur - p_prev) * y_scale`` — with ``start``
    ``d = p_cur * y_scale + y_shift`` — then ``acc += d``, ``sq += d * d`` (uncontracted fp64, one
    thread per cell: a numpy float64 replay bit for bit), and ``p_prev = p_cur``. ``p_cur`` /
    ``p_prev``: distinct fp32 device vectors [M]. Stream-ordered; nothing comes back to the host."""
    import torch

    for name, t in (("p_cur", p_cur), ("p_prev", p_prev)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise TypeError(f"attr_step: {name} must be a float32 tensor, got {getattr(t, 'dtype', type(t))}")
    if p_cur.dim() != 1 or p_cur.shape != p_prev.shape or p_cur.numel() < 1:
        raise ValueError(f"attr_step: p_cur {tuple(p_cur.shape)} and p_prev {tuple(p_prev.shape)} must be equal, "
                         f"non-empty vectors")
    if not p_cur.is_contiguous() or not p_prev.is_contiguous():
        raise ValueError("attr_step: p_cur / p_prev must be contiguous")
    M = p_cur.numel()
    for name, t in (("acc", acc), ("sq", sq)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64:
            raise TypeError(f"attr_step: {name} must be a float64 tensor, got {getattr(t, 'dtype', type(t))}")
        if t.dim() != 2 or t.shape[1] != M or not t.is_contiguous():
            raise ValueError(f"attr_step: {name} must be contiguous float64 [K + 1][{M}], got {tuple(t.shape)}")
    if acc.shape != sq.shape:
        raise ValueError(f"attr_step: acc {tuple(acc.shape)} and sq {tuple(sq.shape)} differ")
    if not (p_cur.device == p_prev.device == acc.device == sq.device) or p_cur.device.type != "cuda":
        raise ValueError(f"attr_step: the tensors must be on one GPU, got {p_cur.device}, {p_prev.device}, "
                         f"{acc.device}, {sq.device}")
    if not 0 <= int(row) < acc.shape[0]:
        raise ValueError(f"attr_step: row {row} outside [0, {acc.shape[0]})")
    lib().attr_step(p_cur, p_prev, float(y_scale), float(y_shift), acc, sq, int(row), bool(start))


SOLVE_FIRST, SOLVE_SCAN, SOLVE_REFINE = 0, 1, 2  # csrc/kernels.h kSolveFirst / kSolveScan / kSolveRefine


def _spans_overlap(t, u) -> bool:
    a0, b0 = t.data_ptr(), u.data_ptr()
    return not (a0 + t.numel() * t.element_size() <= b0 or b0 + u.numel() * u.element_size() <= a0)


def solve_step(p, want, y_scale: float, y_shift: float, mode: int, grid_x, xs, fs, status):
    """One pass of a set-point run (csrc/score.hip; the rule is wellflow/setpoint.py's
    ``solve_step_host``): the residual ``r = p * y_scale + y_shift - want`` in uncontracted fp64
    moves every row's state — ``xs`` float32 [4][M] (lo, hi, best_x, xq), ``fs`` float64 [3][M]
    (f_lo, f_hi, best_r), ``status`` int32 [M] (0 open, 1 bracketed) — one thread per row, bit for
    bit the numpy rule. ``mode``: ``SOLVE_FIRST`` / ``SOLVE_SCAN`` take the pass's value from
    ``grid_x`` (a one-element float32 device tensor: an element of a grid uploaded once),
    ``SOLVE_REFINE`` the row's own ``xq`` (``grid_x`` None). ``p`` / ``want``: float32 device
    vectors [M] that do not overlap the state. Stream-ordered; nothing comes back to the host."""
    import torch

    for name, t in (("p", p), ("want", want)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise TypeError(f"solve_step: {name} must be a float32 tensor, got {getattr(t, 'dtype', type(t))}")
    if p.dim() != 1 or p.shape != want.shape:
        raise ValueError(f"solve_step: p {tuple(p.shape)} and want {tuple(want.shape)} must be equal vectors")
    M = p.numel()
    if M < 1:
        raise ValueError("solve_step: no predictions (M < 1)")
    if int(mode) not in (SOLVE_FIRST, SOLVE_SCAN, SOLVE_REFINE):
        raise ValueError(f"solve_step: mode {mode} is not SOLVE_FIRST (0), SOLVE_SCAN (1) or SOLVE_REFINE (2)")
    for name, t, dt, lead in (("xs", xs, torch.float32, 4), ("fs", fs, torch.float64, 3)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt:
            raise TypeError(f"solve_step: {name} must be a {dt} tensor, got {getattr(t, 'dtype', type(t))}")
        if tuple(t.shape) != (lead, M):
            raise ValueError(f"solve_step: {name} must be [{lead}][{M}], got {tuple(t.shape)}")
    if not isinstance(status, torch.Tensor) or status.dtype != torch.int32:
        raise TypeError(f"solve_step: status must be an int32 tensor, got {getattr(status, 'dtype', type(status))}")
    if tuple(status.shape) != (M,):
        raise ValueError(f"solve_step: status must be [{M}], got {tuple(status.shape)}")
    named = (("p", p), ("want", want), ("xs", xs), ("fs", fs), ("status", status))
    if p.device.type != "cuda" or any(t.device != p.device for _, t in named):
        raise ValueError("solve_step: the tensors must be on one GPU, got " + ", ".join(str(t.device) for _, t in named))
    for name, t in named:
        if not t.is_contiguous():
            raise ValueError(f"solve_step: {name} must be contiguous")
    if int(mode) == SOLVE_REFINE:
        if grid_x is not None:
            raise ValueError("solve_step: a refine pass reads every row's own xq; grid_x must be None")
    else:
        if not isinstance(grid_x, torch.Tensor) or grid_x.dtype != torch.float32:
            raise TypeError(f"solve_step: grid_x must be a float32 tensor, got {getattr(grid_x, 'dtype', type(grid_x))}")
        if grid_x.device != p.device or grid_x.numel() != 1 or not grid_x.is_contiguous():
            raise ValueError(f"solve_step: grid_x must be one contiguous element on {p.device}, got "
                             f"{tuple(grid_x.shape)} on {grid_x.device}")
    for name, t in (("p", p), ("want", want)):
        for sname, st in (("xs", xs), ("fs", fs), ("status", status)):
            if _spans_overlap(t, st):
                raise ValueError(f"solve_step: {name} overlaps the state ({sname})")
    lib().solve_step(p, want, float(y_scale), float(y_shift), int(mode), grid_x, xs, fs, status)


ERR_SUMS_SCRATCH = 2 * 256 + 1  # csrc/kernels.h kErrSumsScratch: a partial pair per workgroup + the ticket


def err_sums_scratch(device):
    """The zeroed scratch block of :func:`err_sums` (one per stream; the kernel leaves it ready
    for its next launch)."""
    import torch

    return torch.zeros(ERR_SUMS_SCRATCH, dtype=torch.float64, device=device)


GROUP_PIECE = 1024  # csrc/kernels.h kGroupPiece: positions per piece; the order of additions depends on it
GROUP_SUMS_MAX_GROUPS = 16384  # csrc/kernels.h kGroupSumsMaxGroups: out is passes x G x 24 bytes


class GroupPlan:
    """How :func:`group_sums` reduces M predictions into G groups: built ONCE per table on the
    host (the grouping is the same for every pass of a run) and uploaded.

    ``ids``: one group id in [0, G) per prediction (any integer array). The plan holds
    ``order`` int32 [M], a stable argsort of the ids (predictions are read through it: the
    identity when they are already grouped); every group's run in ``order`` cut into pieces of at
    most ``GROUP_PIECE`` positions — ``pieces`` int32 [2][P]: first position and length, and
    ``piece_group`` (host, int32 [P]) — ``group_pieces`` int32 [G + 1]: group g owns the pieces
    [group_pieces[g], group_pieces[g + 1]) (none: an empty group); and the scratch buffer
    (fp64 [3 P], no state between launches). ``counts`` (host, int64 [G]): rows per group."""

    def __init__(self, ids, G: int, device):
        import numpy as np
        import torch

        self.device = dev = torch.device(device)
        self.G = G = int(G)
        if not 1 <= G <= GROUP_SUMS_MAX_GROUPS:
            raise ValueError(f"group_sums: {G} groups (need 1 .. {GROUP_SUMS_MAX_GROUPS})")
        ids = np.asarray(ids)
        if ids.ndim != 1 or ids.dtype.kind not in "iu":
            raise TypeError(f"group_sums: the group ids must be a vector of integers, got {ids.dtype} {ids.shape}")
        self.M = M = len(ids)
        if not 1 <= M < 2 ** 31:
            raise ValueError(f"group_sums: {M} predictions (need 1 .. 2^31 - 1)")
        ids = ids.astype(np.int64)
        if ids.min() < 0 or ids.max() >= G:
            bad = ids[(ids < 0) | (ids >= G)][0]
            raise ValueError(f"group_sums: group id {int(bad)} outside [0, {G})")
        order = np.argsort(ids, kind="stable")
        self.counts = counts = np.bincount(ids, minlength=G).astype(np.int64)
        npieces = (counts + GROUP_PIECE - 1) // GROUP_PIECE
        gp = np.concatenate([[0], np.cumsum(npieces)]).astype(np.int64)
        group = np.repeat(np.arange(G, dtype=np.int64), npieces)
        k = np.arange(int(gp[-1]), dtype=np.int64) - gp[group]  # the piece's index inside its group
        first = (np.cumsum(counts) - counts)[group] + k * GROUP_PIECE
        length = np.minimum(GROUP_PIECE, counts[group] - k * GROUP_PIECE)
        self.piece_group = group.astype(np.int32)
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)  # noqa: E731
        self.order, self.pieces, self.group_pieces = i32(order), i32(np.stack([first, length])), i32(gp)
        self.scratch = torch.zeros(3 * int(gp[-1]), dtype=torch.float64, device=dev)


def group_sums(pred, plan: GroupPlan, y_scale: float, y_shift: float, out, slot: int):
    """``out[slot][g] = {n_g, sum v, sum v * v}``, ``v = pred * y_scale + y_shift`` in fp64, per
    group of ``plan`` (csrc/score.hip): ``pred`` fp32 device vector [plan.M], ``out`` fp64
    [S][plan.G][3]. An empty group gives zeros; a NaN prediction makes only its own group's sums
    NaN. No float atomics: bitwise repeatable for a given plan. Stream-ordered; nothing comes back
    to the host."""
    import torch

    if not isinstance(plan, GroupPlan):
        raise TypeError("group_sums: plan must be a GroupPlan")
    if not isinstance(pred, torch.Tensor) or pred.dtype != torch.float32:
        raise TypeError(f"group_sums: pred must be a float32 tensor, got {getattr(pred, 'dtype', type(pred))}")
    if pred.device != plan.device:
        raise ValueError(f"group_sums: pred is on {pred.device}, the plan on {plan.device}")
    if pred.dim() != 1 or pred.numel() != plan.M or not pred.is_contiguous():
        raise ValueError(f"group_sums: pred holds {tuple(pred.shape)} predictions, the plan groups {plan.M}")
    if not isinstance(out, torch.Tensor) or out.dtype != torch.float64:
        raise TypeError(f"group_sums: out must be a float64 tensor, got {getattr(out, 'dtype', type(out))}")
    if out.device != plan.device or out.dim() != 3 or tuple(out.shape[1:]) != (plan.G, 3) or not out.is_contiguous():
        raise ValueError(f"group_sums: out must be float64 [S][{plan.G}][3] on {plan.device}, got {tuple(out.shape)}")
    if not 0 <= int(slot) < out.shape[0]:
        raise ValueError(f"group_sums: slot {slot} outside [0, {out.shape[0]})")
    lib().group_sums(pred, plan.order, plan.pieces, plan.group_pieces, float(y_scale), float(y_shift), out, int(slot),
                     plan.scratch)


def abs_scores(pred, y, y_scale: float, y_shift: float, relative: bool, out):
    """``out[i] = float32(|d|)``, with ``relative`` ``float32(|d| / |v|)``, for ``v = pred * y_scale +
    y_shift`` and ``d = v - y`` in uncontracted fp64 (csrc/quantile.hip; the rule is
    wellflow/interval.py's ``score_host``, bit for bit): the conformal scores of a calibration pass.
    ``pred`` / ``y`` / ``out``: contiguous fp32 device vectors [M]; ``out`` does not overlap the
    other two. Stream-ordered; nothing comes back to the host."""
    import torch

    named = (("pred", pred), ("y", y), ("out", out))
    for name, t in named:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise TypeError(f"abs_scores: {name} must be a float32 tensor, got {getattr(t, 'dtype', type(t))}")
    if pred.dim() != 1 or pred.numel() < 1:
        raise ValueError(f"abs_scores: pred {tuple(pred.shape)} must be a non-empty vector")
    for name, t in named[1:]:
        if t.shape != pred.shape:
            raise ValueError(f"abs_scores: {name} {tuple(t.shape)} must have pred's shape {tuple(pred.shape)}")
    if pred.device.type != "cuda" or any(t.device != pred.device for _, t in named):
        raise ValueError("abs_scores: the tensors must be on one GPU, got " + ", ".join(str(t.device) for _, t in named))
    for name, t in named:
        if not t.is_contiguous():
            raise ValueError(f"abs_scores: {name} must be contiguous")
    for name, t in named[:2]:
        if _spans_overlap(t, out):
            raise ValueError(f"abs_scores: out overlaps {name}")
    lib().abs_scores(pred, y, float(y_scale), float(y_shift), bool(relative), out)


QUANTILE_MAX_LEVELS = 4  # csrc/kernels.h kQuantMaxLevels
QUANTILE_MAX_CELLS = 16384  # csrc/kernels.h kQuantMaxCells: hist is G x A x 1 KiB, at most 16 MiB


class QuantilePlan:
    """How :func:`group_quantiles` selects ``A`` order statistics in each of ``G`` groups of M
    scores: a :class:`GroupPlan` of the ids (``groups``: built once on the host, as for the grouped
    sums), the group of every piece on the device (``piece_group``), and the select's working
    memory: ``hist`` int32 [G][A][256], zero here and left zero by every call, and ``state`` int32
    [G][A][2] (the key prefix and the remaining rank of a (group, level), written before it is
    read). ``1 <= A <= QUANTILE_MAX_LEVELS`` and ``G * A <= QUANTILE_MAX_CELLS``."""

    def __init__(self, ids, G: int, A: int, device):
        import torch

        G, A = int(G), int(A)
        if not 1 <= A <= QUANTILE_MAX_LEVELS:
            raise ValueError(f"group_quantiles: {A} levels (need 1 .. {QUANTILE_MAX_LEVELS})")
        if G < 1 or G * A > QUANTILE_MAX_CELLS:
            raise ValueError(f"group_quantiles: {G} groups x {A} levels = {G * A} histograms (need 1 .. "
                             f"{QUANTILE_MAX_CELLS}: 1 KiB each, 16 MiB in all)")
        self.groups = GroupPlan(ids, G, device)
        self.G, self.A, self.M, self.device, self.counts = G, A, self.groups.M, self.groups.device, self.groups.counts
        self.piece_group = torch.from_numpy(self.groups.piece_group).to(self.device)
        self.hist = torch.zeros((G, A, 256), dtype=torch.int32, device=self.device)
        self.state = torch.zeros((G, A, 2), dtype=torch.int32, device=self.device)


def group_quantiles(scores, plan: QuantilePlan, ranks, out):
    """``out[g][a]`` = the ``ranks[g][a]``-th smallest (0-based, clamped into the group) of the scores
    of group ``g`` of ``plan``, exactly (csrc/quantile.hip): ``np.sort`` per group bit for bit for
    scores that are non-negative or NaN (NaN sorts last); NaN for an empty group. ``scores`` fp32
    device vector [plan.M], ``ranks`` int32 [plan.G][plan.A] and ``out`` fp32 [plan.G][plan.A] on the
    plan's device. Integer atomics only: bitwise repeatable; a NaN score moves only its own group's
    answers. Stream-ordered; nothing comes back to the host."""
    import torch

    if not isinstance(plan, QuantilePlan):
        raise TypeError("group_quantiles: plan must be a QuantilePlan")
    for name, t, dt in (("scores", scores, torch.float32), ("ranks", ranks, torch.int32), ("out", out, torch.float32)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt:
            raise TypeError(f"group_quantiles: {name} must be a {dt} tensor, got {getattr(t, 'dtype', type(t))}")
        if t.device != plan.device:
            raise ValueError(f"group_quantiles: {name} is on {t.device}, the plan on {plan.device}")
    if scores.dim() != 1 or scores.numel() != plan.M or not scores.is_contiguous():
        raise ValueError(f"group_quantiles: scores holds {tuple(scores.shape)} scores, the plan groups {plan.M}")
    for name, t in (("ranks", ranks), ("out", out)):
        if tuple(t.shape) != (plan.G, plan.A) or not t.is_contiguous():
            raise ValueError(f"group_quantiles: {name} must be contiguous [{plan.G}][{plan.A}] (groups x levels), "
                             f"got {tuple(t.shape)}")
    if _spans_overlap(scores, out):
        raise ValueError("group_quantiles: out overlaps scores")
    g = plan.groups
    lib().group_quantiles(scores, g.order, g.pieces, plan.piece_group, ranks, plan.hist, plan.state, out)


def gemm(A, B, M, N, K, *, a_mn=False, lda=None, b_mn=False, ldb=None, outF=None, outH=None,
         ldo=None, bias=None, mask=None, ldm=None, mask_scale=1.0, colsum=None, alpha=1.0,
         beta=0.0, act=0, atomic=False, ksplit=1, drop_p=0.0, seed=0, tile=0, seed_dev=None):
    """out = act(alpha * A(M,K) B(N,K)^T + beta*out + bias) (* mask), on MFMA.

    ``a_mn``/``b_mn`` select the MN-contiguous layout (X(r,k) = p[k*ld + r]).
    ``tile`` (MN x MN split-K atomic only; csrc/kernels.h DwTile): 0 = the generic 128x128
    kernels, 1 = 256x128, 3 = 256x192 (N % 192 == 0, else 256x128), 4 / 5 = 3 through a 5- /
    4-slot half-step ring (A/B), 7 = the best for N (256x288, else 256x192, else 256x128). Any
    other id raises; a shape the tile cannot take runs as 0.
    ``seed_dev`` (int64 GPU tensor): a device step counter mixed into the dropout seed.

    Order of the epilogue: ``alpha * acc``, ``+ beta * out``, ``+ bias``, ReLU (``act`` 1),
    dropout (``drop_p`` in [0, 1), key ``m * N + n``), mask (``mask > 0`` keeps, times
    ``mask_scale``). ``outF`` and ``outH`` may be given together; ``outH`` is rounded to nearest
    even. Pinned bit for bit by tests/test_gemm_exact_gpu.py, with these rules:

    * ``colsum[n] +=`` the column sums of what the epilogue has in hand: the staged bf16 epilogue
      (``outH`` alone, ``beta`` 0, ``N``, ``ldo`` and ``ldm`` multiples of 8) sums the
      bf16-ROUNDED values it stores, the direct epilogue (every other call) the UNROUNDED fp32
      values, also when only ``outH`` is written. The two agree whenever the outputs are bf16
      numbers; :func:`gemm_plan` tells which one a call takes.
    * ``atomic`` adds ``alpha * acc`` into ``outF`` and nothing else: ``bias``, ``mask``,
      ``colsum``, ``act`` and ``drop_p`` raise together with it (they used to be ignored).
    * ``act`` outside {0, 1} and ``drop_p`` outside [0, 1) raise.
    """
    lib().gemm(*_gemm_args(A, B, M, N, K, a_mn, lda, b_mn, ldb, outF, outH, ldo, bias, mask, ldm, mask_scale, colsum,
                           alpha, beta, act, atomic, ksplit, drop_p, seed, tile, seed_dev))


def gemm_plan(A, B, M, N, K, *, a_mn=False, lda=None, b_mn=False, ldb=None, outF=None, outH=None,
              ldo=None, bias=None, mask=None, ldm=None, mask_scale=1.0, colsum=None, alpha=1.0,
              beta=0.0, act=0, atomic=False, ksplit=1, drop_p=0.0, seed=0, tile=0, seed_dev=None) -> dict:
    """The route :func:`gemm` takes for the same arguments, after the same checks, without a
    launch: ``kernel`` ("generic", "dw256x128", "dw256x192", "dw256x192h", "dw256x288"),
    ``mainloop`` ("ring" = direct-to-LDS, "register"), ``epilogue`` ("staged", "direct"),
    ``kchunk``, ``nsplit``, ``workgroups``. It is the function the launcher itself calls
    (csrc/kernels.h gemm_plan). Tensors on the CPU are accepted: only their sizes count."""
    return lib().gemm_plan(*_gemm_args(A, B, M, N, K, a_mn, lda, b_mn, ldb, outF, outH, ldo, bias, mask, ldm,
                                       mask_scale, colsum, alpha, beta, act, atomic, ksplit, drop_p, seed, tile,
                                       seed_dev))


def _gemm_args(A, B, M, N, K, a_mn, lda, b_mn, ldb, outF, outH, ldo, bias, mask, ldm, mask_scale, colsum, alpha,
               beta, act, atomic, ksplit, drop_p, seed, tile, seed_dev) -> tuple:
    if lda is None:
        lda = M if a_mn else K
    if ldb is None:
        ldb = N if b_mn else K
    if ldo is None:
        ldo = N
    if ldm is None:
        ldm = ldo
    return (A, bool(a_mn), int(lda), B, bool(b_mn), int(ldb), int(M), int(N), int(K), int(ksplit), outF, outH,
            int(ldo), bias, mask, int(ldm), float(mask_scale), colsum, float(alpha), float(beta), int(act),
            bool(atomic), float(drop_p), int(seed), int(tile), seed_dev)
