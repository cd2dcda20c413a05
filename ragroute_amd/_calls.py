"""The one Python call layer in front of the C ABI's search path: what FlatIndex, SegmentedIndex (flat_index.py) and the custom ops
(torch_ops.py) all need before and around a library call, each piece once.  PyTorch is memory and streams only; nothing here
synchronises with the host, guards a device or keeps state of its own (a workspace cache belongs to its caller)."""
import numpy as np
import torch

from . import _lib
from ._lib import check, lib

TORCH_DTYPE = {"fp16": torch.float16, "bf16": torch.bfloat16}
RR_DTYPE = {"fp16": _lib.RR_DTYPE_F16, "bf16": _lib.RR_DTYPE_BF16, torch.float16: _lib.RR_DTYPE_F16, torch.bfloat16: _lib.RR_DTYPE_BF16}


def dtype_code(t):
    """RR_DTYPE_* of a half tensor."""
    code = RR_DTYPE.get(t.dtype)
    if code is None:
        raise ValueError("corpus / queries must be float16 or bfloat16")
    return code


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def require_gpu():
    if not torch.cuda.is_available():
        raise _lib.RagrouteHipError("ragroute_amd needs a HIP device (torch.cuda.is_available() is False); there is no CPU fallback")


def f32_rows(part, device):
    """A chunk of f32 rows (numpy, np.memmap or tensor) as a contiguous float32 tensor on `device`."""
    if isinstance(part, np.ndarray):  # also np.memmap: only this chunk is paged in
        part = np.ascontiguousarray(part, dtype=np.float32)
        part = torch.from_numpy(part if part.flags.writeable else part.copy())
    return part.to(device, dtype=torch.float32).contiguous()


def f32_queries(xq, d, device):
    """float32 [nq,d] queries (numpy or tensor) as a contiguous float32 tensor on `device`."""
    if isinstance(xq, np.ndarray):
        xq = torch.from_numpy(np.ascontiguousarray(xq, dtype=np.float32))
    if xq.dim() != 2 or xq.shape[1] != d:
        raise ValueError(f"queries must be [nq,{d}]")
    return xq.to(device, dtype=torch.float32).contiguous()


def l2_normalize_(x):
    """rr_l2_normalize_f32: contiguous device f32 rows [n,d], normalised in place."""
    check(lib().rr_l2_normalize_f32(x.data_ptr(), x.shape[0], x.shape[1], stream_ptr()), "rr_l2_normalize_f32")


def rows_to_half(x, dim, dtype, normalize, out=None):
    """rr_rows_to_half: contiguous device f32 rows [n,d] -> [n,dim] of torch dtype `dtype`, zero padded, into `out` or a fresh tensor."""
    n, d = x.shape
    if out is None:
        out = torch.empty((n, dim), dtype=dtype, device=x.device)
    check(lib().rr_rows_to_half(x.data_ptr(), n, d, d, out.data_ptr(), RR_DTYPE[dtype], dim, int(normalize), stream_ptr()), "rr_rows_to_half")
    return out


def half_sqnorms(xb, n_rows, out=None):
    """rr_half_sqnorms: |x|^2 / 2 of the first n_rows rows of the half matrix xb, into `out` or a fresh f32 vector."""
    if out is None:
        out = torch.empty(max(1, n_rows), dtype=torch.float32, device=xb.device)
    check(lib().rr_half_sqnorms(xb.data_ptr(), dtype_code(xb), n_rows, xb.shape[1], out.data_ptr(), stream_ptr()), "rr_half_sqnorms")
    return out


def check_half_queries(xq_half, dtype, dim, message):
    """Prepared queries are a contiguous [nq, dim] matrix of the corpus dtype."""
    if xq_half.dtype != dtype or xq_half.dim() != 2 or xq_half.shape[1] != dim or not xq_half.is_contiguous():
        raise ValueError(message)


def out_pair(nq, k, device, out=None):
    """(D f32 [nq,k], I i64 [nq,k]): the caller's `out`, or fresh tensors."""
    if out is not None:
        D, I = out
        return D, I
    return torch.empty((nq, k), dtype=torch.float32, device=device), torch.empty((nq, k), dtype=torch.int64, device=device)


def workspace(cache, key, device, message, size_query, *args):
    """The one-entry workspace cache: `cache` (a dict its owner keeps) holds the buffer of the last key; another key replaces it with
    one of lib().<size_query>(*args) bytes.  A size of 0 is the library's word for arguments out of range: ValueError of `message`,
    formatted with args.  (The query is named and the message a template so that a hit costs one dict lookup.)"""
    ws = cache.get(key)
    if ws is None:
        nbytes = getattr(lib(), size_query)(*args)
        if nbytes == 0:
            raise ValueError(message.format(*args))
        cache.clear()
        ws = cache[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return ws


def half_search(xb, n_rows, xq_half, k, D, I, ws, mptr, mstride, id_offset=0, segs=None, l2=False, hn=None):
    """The half-precision search of n_rows rows of xb [*, dim] for the prepared queries xq_half [nq, dim] into D, I: rr_flat_search, or
    rr_flat_search_segments when a segment table is given (ids then come from the table, not id_offset); l2: their squared-L2 forms
    with the half squared norms hn (None, the null pointer, serves an L2 index that is still empty)."""
    code, dim, nq = dtype_code(xb), xb.shape[1], xq_half.shape[0]
    if segs is None:
        if l2:
            check(lib().rr_flat_search_l2(xb.data_ptr(), hn.data_ptr() if hn is not None else None, code, n_rows, dim, xq_half.data_ptr(), nq,
                                          k, D.data_ptr(), I.data_ptr(), id_offset, ws.data_ptr(), ws.numel(), mptr, mstride, stream_ptr()),
                  "rr_flat_search_l2")
        else:
            check(lib().rr_flat_search(xb.data_ptr(), code, n_rows, dim, xq_half.data_ptr(), nq, k, D.data_ptr(), I.data_ptr(), id_offset,
                                       ws.data_ptr(), ws.numel(), mptr, mstride, stream_ptr()), "rr_flat_search")
    elif l2:
        check(lib().rr_flat_search_segments_l2(xb.data_ptr(), hn.data_ptr() if hn is not None else None, code, n_rows, dim, segs, len(segs),
                                               xq_half.data_ptr(), nq, k, D.data_ptr(), I.data_ptr(), ws.data_ptr(), ws.numel(), mptr, mstride,
                                               stream_ptr()), "rr_flat_search_segments_l2")
    else:
        check(lib().rr_flat_search_segments(xb.data_ptr(), code, n_rows, dim, segs, len(segs), xq_half.data_ptr(), nq, k, D.data_ptr(),
                                            I.data_ptr(), ws.data_ptr(), ws.numel(), mptr, mstride, stream_ptr()), "rr_flat_search_segments")
