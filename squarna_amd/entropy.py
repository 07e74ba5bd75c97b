"""``Entropy``: the reference's entropy mode as data.

``Predict(entropy=True)`` prints one rounded number per record: the mean row entropy of the record's stem matrix
(SQRNdbnseq.py:520-545, 1087-1089).  ``Entropy`` takes the same inputs and returns an :class:`EntropyResult`: the entropy of
EVERY row -- one value per position, which is what one plots or feeds to a model -- and the unrounded mean, as torch tensors.
With the GPU engine all records of a call go through the batch engine in chunks and the rows are formed by kernels
(``sq_entropy_rows``); nothing but sizes and offsets leaves the device.  ``Entropy`` prints nothing.
"""
import numpy as np

from . import engine as _engine
from . import fold as _fold
from .dbn import gap_mask
from .options import as_float, check_sources, configs_by_length, input_records, pick
from .results import TensorResult
from .rows import offsets


class EntropyResult(TensorResult):
    """Row entropies of ``Entropy`` for R records.

    Host lists: ``names``, ``sequences`` (as given), ``paramset_names`` (per record: the paramset used).  ``source``: "device"
    or "host" -- where the rows were formed.  Torch tensors (``device``: where they live): ``lengths`` int64[R] and
    ``pos_off`` int64[R + 1]; ``position`` float64[sum of lengths] -- record r from pos_off[r] on, one value per column of the
    sequence AS GIVEN: the entropy H_i in bits of that position's row of the stem matrix, NaN at a gap column, 0.0 where the
    row is empty (a separator, a position no stem covers); ``mean`` float64[R]: sum H_i / N over the record's N gap-free
    positions, separators counted -- the reference's value before it is rounded; NaN for a record without a position;
    ``nstems`` int32[R]: the stems that formed the matrix."""

    _TENSORS = ("position", "lengths", "pos_off", "mean", "nstems")

    def __init__(self, names, sequences, paramset_names, tables, source):
        self.names, self.sequences, self.paramset_names, self.source = names, sequences, paramset_names, source
        self.position, self.lengths, self.pos_off, self.mean, self.nstems = (tables[k] for k in self._TENSORS)
        self._lengths = np.array([len(s) for s in sequences], np.int64)      # the host's copy of the sizes
        self._pos_off = offsets(self._lengths)

    def __len__(self):
        return len(self.names)

    def row(self, r):
        """Record r's values, one per column of its sequence as given: a view of ``position``."""
        return self.position[int(self._pos_off[r]):int(self._pos_off[r + 1])]

    def text(self, r):
        """The string the reference prints for record r (SQRNdbnseq.py:545)."""
        return str(round(float(self.mean[r]), 3))

    def to_padded(self):
        """float64[R, Lmax]: every record's values, NaN where a record is shorter; formed on the tensors' device."""
        import torch
        R, Lmax, total = len(self.names), int(self._lengths.max(initial=0)), int(self._pos_off[-1])
        out = torch.full((R, Lmax), float("nan"), dtype=torch.float64, device=self.device)
        if total:
            rec = torch.repeat_interleave(torch.arange(R, device=self.device), self.lengths, output_size=total)
            out[rec, torch.arange(total, device=self.device) - self.pos_off[rec]] = self.position
        return out


def _stem_matrix(stem_matrix, on_device):
    """Entropy's stem_matrix argument as a square float64 matrix: a contiguous CUDA tensor for the GPU engine (one that is there
    already is used where it is), a numpy array otherwise."""
    import torch
    m = stem_matrix if hasattr(stem_matrix, "is_cuda") else torch.from_numpy(np.ascontiguousarray(stem_matrix))
    if m.dim() != 2 or m.shape[0] != m.shape[1]:
        raise ValueError("stem_matrix: shape %s; a square [L, L] matrix is needed" % (tuple(m.shape),))
    if m.dtype != torch.float64:
        raise ValueError("stem_matrix: dtype %s; float64 is needed" % m.dtype)
    if not on_device:
        return m.detach().cpu().numpy()
    if not m.is_cuda:
        m = m.to(torch.device("cuda", torch.cuda.current_device()))
    return m if m.is_contiguous() else m.contiguous()


def Entropy(inputfile=None, fileformat="unknown", inputseq=None, configfile=None, inputformat="qtrf",
            interchainonly=False, ignorewarn=False, HOME_DIR=None, M=1.8, B=-0.6, records=None,
            paramset=0, stem_matrix=None, bpp=None, inputrestr=None,
            i=None, ff=None, c=None, config=None, s=None, seq=None, ico=None, iw=None, ignore=None):
    """The row entropies of every input record's stem matrix as an :class:`EntropyResult`.

    The inputs (``inputfile`` / ``inputseq`` / ``records``), their synonyms, validation messages and the choice of
    configuration by length when no ``configfile`` is given are ``Fold``'s.  ``paramset``: the paramset of the record's
    configuration the stems are formed under, by index or by name; 0 is what the reference uses.

    ``stem_matrix``: an ``[L, L]`` float64 tensor (CUDA or CPU) or array over the columns of the input as given; it multiplies
    the pair scores of every record through the record's gap map (the reference's ``stemmatrix`` argument,
    SQRNdbnseq.py:1031-1034, 1084-1085), as given, without normalisation (``FoldAlignment(...).stem_matrix`` is normalised
    already).  All records must then have L columns.  A CUDA tensor is read where it is and is not modified.
    ``bpp``: as for ``Fold``; needed only when the paramset has ``bpp != 0``.

    The stems are ``AnnotateStems`` with no stem selected: every cell of a stem and its mirror hold the stem's total score,
    and row i with S = sum_j m[i][j] != 0 has H_i = -sum p log2 p over its nonzero cells, p = m[i][j] / S (else 0)."""
    import torch
    inputfile = pick(inputfile, i); fileformat = pick(fileformat, ff)
    configfile = pick(configfile, config, c); inputseq = pick(inputseq, seq, s)
    interchainonly = pick(interchainonly, ico); ignorewarn = pick(ignorewarn, ignore, iw)
    inputfile, configfile, configfileset, _, HOME_DIR = check_sources(records, inputfile, inputseq, fileformat, configfile,
                                                                             inputformat, HOME_DIR, None)
    M, B = as_float(M, "M"), as_float(B, "B")
    config_for = configs_by_length(configfile, configfileset, HOME_DIR)
    inputs = input_records(records, inputseq, inputfile, inputformat, fileformat, ignorewarn, inputrestr, M, B)

    eng = _engine.get_engine()
    if not hasattr(eng, "entropy_tensors"):
        raise RuntimeError("Entropy needs an engine with entropy_tensors; the %s engine has none"
                           % getattr(eng, "name", type(eng).__name__))
    seqs = [rec[1] for rec in inputs]
    used, names = [], []
    for sq in seqs:
        psnames, psets = config_for(sq)
        k = paramset
        if isinstance(k, str):
            if k not in psnames:
                raise ValueError("Unknown paramset {!r}; the configuration has: {}".format(k, ", ".join(psnames)))
            k = psnames.index(k)
        elif isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= k < len(psets):
            raise ValueError("Unknown paramset {!r}; the configuration has {} paramsets".format(paramset, len(psets)))
        used.append(psets[k])
        names.append(psnames[k])
    on_device = getattr(eng, "name", None) == "hip"               # (another engine, the tests' CPU one, takes host arrays)
    if stem_matrix is not None:
        stem_matrix = _stem_matrix(stem_matrix, on_device)
        bad = [k for k, sq in enumerate(seqs) if len(sq) != stem_matrix.shape[0]]
        if bad:
            raise ValueError("stem_matrix: {0} x {0} for record {1} ({2}) of {3} columns; every record needs {0}".format(
                int(stem_matrix.shape[0]), bad[0], inputs[bad[0]][0], len(seqs[bad[0]])))
    mats = _fold._bpp_matrices(bpp, seqs, on_device) if bpp is not None else None
    t = eng.entropy_tensors([(rec[1], rec[2], rec[3], ps) for rec, ps in zip(inputs, used)], interchainonly=interchainonly, M=M, B=B,
                            stem_matrix=stem_matrix, bpp=mats)

    # gap-free coordinates -> columns of the sequences as given: NaN at the gap columns
    dev = t["position"].device
    lengths = np.array([len(sq) for sq in seqs], np.int64)
    pos_off = offsets(lengths)
    if (np.asarray(t["lengths"], np.int64) == lengths).all():
        position = t["position"]
    else:
        where = np.concatenate([np.flatnonzero(~gap_mask(sq)) + o for sq, o in zip(seqs, pos_off[:-1])])
        position = torch.full((int(pos_off[-1]),), float("nan"), dtype=torch.float64, device=dev)
        position[torch.from_numpy(where).to(dev)] = t["position"]
    tables = dict(lengths=torch.from_numpy(lengths).to(dev), pos_off=torch.from_numpy(pos_off).to(dev), position=position,
                  mean=t["mean"], nstems=t["nstems"])
    return EntropyResult([rec[0] for rec in inputs], seqs, names, tables, "device" if position.is_cuda else "host")
