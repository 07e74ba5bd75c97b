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
    """Replace the source of base-pair probabilities (fn(shortseq, reacts, M, B) -> N x N array or None)."""
    global _bpp_provider
    old, _bpp_provider = _bpp_provider, (fn or vienna_bpp)
    return old


def bpp_terms(prepared, psets, M=1.8, B=-0.6):
    """Per job (record-major, paramset-minor) the dense term the fill applies for bpp != 0 paramsets:
    (bppm / max(bppm)) ** |bpp|  (SQRNdbnseq.py:350-354), or None.  Returns None when no paramset needs one."""
    if not any(ps.get("bpp", 0) for pl in psets for ps in pl):
        return None
    out = []
    for p, pl in zip(prepared, psets):
        bppm = None
        if any(ps.get("bpp", 0) for ps in pl):
            bppm = _bpp_provider(p.shortseq, p.shortreacts if p.shortreacts is not None else [0.5] * len(p.shortseq), M, B)    # once per sequence
            if bppm is not None:
                bppm = np.asarray(bppm, dtype=np.float64)
        for ps in pl:
            power = ps.get("bpp", 0)
            if power and bppm is not None:
                out.append(np.ascontiguousarray((bppm / np.max(bppm)) ** abs(power)))
            else:
                out.append(None)
    return out
