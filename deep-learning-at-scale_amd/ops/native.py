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
    row table (``out``: write into this tensor). The block spec is checked here, on the host, before
    anything is launched."""
    import numpy as np
    import torch

    dev = torch.device(device)
    F = int(n_features)
    off = np.asarray(cat_off, dtype=np.int64).reshape(-1)
    size = np.asarray(cat_size, dtype=np.int64).reshape(-1)
    codes = torch.as_tensor(codes)
    cont = torch.as_tensor(cont)
    C, Q = (codes.shape[0] if codes.numel() else 0), (cont.shape[0] if cont.numel() else 0)
    N = codes.shape[1] if C else (cont.shape[1] if Q else 0)
    if len(off) != C or len(size) != C:
        raise ValueError(f"assemble_features: {C} code columns but {len(off)} offsets / {len(size)} sizes")
    if C and ((size < 0).any() or (off != np.cumsum(size) - size).any()):
        raise ValueError("assemble_features: one-hot blocks must be back to back from column 0")
    if int(size.sum()) + Q != F:
        raise ValueError(f"assemble_features: one-hot width {int(size.sum())} + {Q} continuous != F = {F}")
    if Q and (cont.shape[1] != N or len(mean) != Q or len(std) != Q):
        raise ValueError("assemble_features: cont / mean / std shapes disagree")
    i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32)).to(dev)  # noqa: E731
    f32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dev)  # noqa: E731
    ld = (F + 7) // 8 * 8 if out_dtype == torch.bfloat16 else F
    if N < 1:
        return torch.zeros((0, ld), dtype=out_dtype, device=dev)
    if out is None:
        out = torch.empty((N, ld), dtype=out_dtype, device=dev)
    elif out.shape != (N, ld) or out.dtype != out_dtype:
        raise ValueError(f"assemble_features: out must be {out_dtype} [{N}][{ld}]")
    lib().assemble_features(codes.to(dev, torch.int32).contiguous() if C else None,
                            cont.to(dev, torch.float32).contiguous() if Q else None,
                            i32(off) if C else None, i32(size) if C else None,
                            f32(mean) if Q else None, f32(std) if Q else None, N, F, out)
    return out


def gemm(A, B, M, N, K, *, a_mn=False, lda=None, b_mn=False, ldb=None, outF=None, outH=None,
         ldo=None, bias=None, mask=None, ldm=None, mask_scale=1.0, colsum=None, alpha=1.0,
         beta=0.0, act=0, atomic=False, ksplit=1, drop_p=0.0, seed=0, tile=0, seed_dev=None):
    """out = act(alpha * A(M,K) B(N,K)^T + beta*out + bias) (* mask), on MFMA.

    ``a_mn``/``b_mn`` select the MN-contiguous layout (X(r,k) = p[k*ld + r]).
    ``tile`` (MN x MN split-K atomic only): 1 = 256x128 8-wave tile, 2 = 128x288, 3 = 256x192.
    ``seed_dev`` (int64 GPU tensor): a device step counter mixed into the dropout seed.
    """
    if lda is None:
        lda = M if a_mn else K
    if ldb is None:
        ldb = N if b_mn else K
    if ldo is None:
        ldo = N
    if ldm is None:
        ldm = ldo
    lib().gemm(A, bool(a_mn), int(lda), B, bool(b_mn), int(ldb), int(M), int(N), int(K),
               int(ksplit), outF, outH, int(ldo), bias, mask, int(ldm), float(mask_scale), colsum,
               float(alpha), float(beta), int(act), bool(atomic), float(drop_p), int(seed), int(tile), seed_dev)
