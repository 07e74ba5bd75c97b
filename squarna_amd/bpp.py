"""Base-pair probabilities from the host (ViennaRNA, or the provider a caller installs) and the dense term the fill applies
for bpp != 0 paramsets."""
import numpy as np

from .dbn import SEPS, ProcessReacts


def vienna_bpp(shortseq, reacts, M=1.8, B=-0.6):
    """Base-pair probability matrix of one sequence exactly as the reference obtains it (SQRNdbnseq.py:342-364):
    ViennaRNA's partition function (with SHAPE pseudo-energies when reactivities are given), rescaled once when all
    probabilities vanish.  Host-side third-party code, outside the accelerated path; None when max(bppm) == 0."""
    try:
        import RNA
    except ImportError:
        raise RuntimeError("this configuration has bpp != 0 paramsets, which need ViennaRNA's Python module `RNA` "
                           "on the host (SQRNdbnseq.py:341-364); it is not installed. Use a config without bpp "
                           "(e.g. c=nobpp) or install ViennaRNA.") from None
    fc = RNA.fold_compound(''.join(ch if ch not in SEPS and ord(ch) <= 127 else 'N' for ch in shortseq))
    if reacts is not None and set(reacts) != {0.5}:
        fc.sc_add_SHAPE_deigan(ProcessReacts(list(reacts), reverse=True, M=M, B=B), m=M, b=B)
    fc.pf()
    bppm = np.array(fc.bpp())[1:, 1:]
    if np.max(bppm) > 0:
        return bppm
    (ss, mfe) = fc.mfe()
    fc.exp_params_rescale(mfe)
    fc.pf()
    bppm = np.array(fc.bpp())[1:, 1:]
    return bppm if np.max(bppm) > 0 else None


_bpp_provider = vienna_bpp


def set_bpp_provider(fn):
    """Replace the source of base-pair probabilities (fn(shortseq, reacts, M, B) -> N x N array or None).
    The provider may also return a CUDA float64 torch tensor (N x N, unit column stride): the record then takes the device
    path of bpp_terms -- its matrix is handed to the batch as it is and the terms are formed on the GPU."""
    global _bpp_provider
    old, _bpp_provider = _bpp_provider, (fn or vienna_bpp)
    return old


def check_bpp_matrix(m, n, what="bpp matrix"):
    """ValueError unless m is what the batch takes as a record's device matrix of base-pair probabilities: a CUDA float64
    2-D torch tensor of n x n elements with unit column stride and a row stride >= n (a view of a larger tensor is fine)."""
    import torch
    if not getattr(m, "is_cuda", False):
        raise ValueError("%s: a CUDA tensor is needed, got %s" % (what, "a CPU tensor" if hasattr(m, "is_cuda") else type(m).__name__))
    if m.dtype != torch.float64:
        raise ValueError("%s: dtype %s, torch.float64 is needed" % (what, m.dtype))
    if m.dim() != 2 or tuple(m.shape) != (n, n):
        raise ValueError("%s: shape %s, the record needs %d x %d (its gap-free length, separators counted)" % (what, tuple(m.shape), n, n))
    if n > 1 and (m.stride(1) != 1 or m.stride(0) < n):
        raise ValueError("%s: strides %s; a unit column stride and a row stride >= %d are needed" % (what, tuple(m.stride()), n))


def device_exponent(power):
    """Whether the device forms the term for this bpp value: |bpp| 0.5 (an IEEE square root) or 1.  Other exponents keep the
    host term, because the host libm's pow is the rule for them."""
    return abs(power) in (0.5, 1.0)


def bpp_terms(prepared, psets, M=1.8, B=-0.6, given=None, device=False):
    """Per job (record-major, paramset-minor) the dense term the fill applies for bpp != 0 paramsets:
    (bppm / max(bppm)) ** |bpp|  (SQRNdbnseq.py:350-354), or None.  Returns None when no paramset needs one.
    given: per record a matrix of probabilities that takes the provider's place (a CUDA float64 tensor or an array), or None.
    device=True: returns (terms, matrices) -- a record whose probabilities are a CUDA tensor (given, or returned by the provider)
    and whose bpp paramsets all have |bpp| 0.5 or 1 gets no host terms; its tensor comes back in `matrices` (per record, else
    None; None when no record has one) and the batch forms the terms on the device (Batch(bpp_dev=...)).  A record with any
    other exponent has its tensor copied to the host ONCE and takes the host terms.  device=False: every tensor is copied to the
    host, the result is the list of terms alone."""
    if not any(ps.get("bpp", 0) for pl in psets for ps in pl):
        return (None, None) if device else None
    out, mats = [], []
    for k, (p, pl) in enumerate(zip(prepared, psets)):
        bppm, dev = None, None
        if any(ps.get("bpp", 0) for ps in pl):
            bppm = given[k] if given is not None and given[k] is not None else None
            mine = bppm is not None
            if bppm is None:
                bppm = _bpp_provider(p.shortseq, p.shortreacts if p.shortreacts is not None else [0.5] * len(p.shortseq), M, B)    # once per sequence
            if bppm is not None and hasattr(bppm, "is_cuda"):             # a torch tensor
                n = len(p.shortseq)
                if bppm.is_cuda:
                    check_bpp_matrix(bppm, n, "bpp matrix of record %d" % k)
                    if device and all(device_exponent(ps.get("bpp", 0)) for ps in pl if ps.get("bpp", 0)):
                        dev, bppm = bppm, None
                if bppm is not None:
                    bppm = bppm.detach().cpu().numpy()
                    mine = True
            if bppm is not None:
                bppm = np.asarray(bppm, dtype=np.float64)
                if mine and (bppm.shape != (len(p.shortseq),) * 2):
                    raise ValueError("bpp matrix of record %d: shape %s, the record needs %d x %d" % (k, bppm.shape, len(p.shortseq), len(p.shortseq)))
                if mine and not np.max(bppm, initial=0.0) > 0:             # (:350,360: the matrix stays as it is)
                    bppm = None
        mats.append(dev)
        for ps in pl:
            power = ps.get("bpp", 0)
            if power and bppm is not None:
                out.append(np.ascontiguousarray((bppm / np.max(bppm)) ** abs(power)))
            else:
                out.append(None)
    if not device:
        return out
    return out, (mats if any(m is not None for m in mats) else None)
