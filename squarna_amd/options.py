"""Predict's keyword surface, once: synonyms, where the input and the configuration come from, the checks of the prediction
keywords with the reference's messages (SQUARNA.py:602-808), alignment mode's default lines, the choice of configuration by
length, the record batches and the parsed input records.  ``Predict``, ``Fold`` and ``FoldAlignment`` resolve their keywords
here, ``Entropy`` its sources; ``FoldWindows``, ``FoldMutants`` and ``FoldDuplex`` open with ``derived_inputs``.
"""
import contextlib
import io
import os

from .config import ParseConfig, DATA_DIR
from .dbn import ProcessReacts, ReactDict
from .inputs import ParseInput


def pick(cur, *alts):
    """A keyword's value: the last of its synonyms that was given, else the keyword itself (SQUARNA.py:602-664)."""
    for alt in alts:
        if alt is not None:
            cur = alt
    return cur


def find_config(configfile, HOME_DIR, priority):
    """(configuration file, whether the caller named one, priority names): SQUARNA.py:683-703.  No file named: def.conf (and, by
    length, 500.conf / 1000.conf beside it) with the default priority paramsets."""
    if configfile is None:
        priority = set('bppN,bppH1,bppH2'.split(',')) if priority is None else {x for x in priority.split(',') if x}
        return os.path.join(HOME_DIR, "def.conf"), False, priority
    if not os.path.exists(configfile):
        if os.path.exists(os.path.join(HOME_DIR, configfile + ".conf")):
            configfile = os.path.join(HOME_DIR, configfile + ".conf")
        elif os.path.exists(os.path.join(HOME_DIR, configfile)):
            configfile = os.path.join(HOME_DIR, configfile)
    assert os.path.exists(configfile), "Config file does not exist."
    return configfile, True, set() if priority is None else {x for x in priority.split(',') if x}


def check_input(records, inputfile, inputseq, fileformat, HOME_DIR=None):
    """Predict's checks of where the input comes from, same messages (SQUARNA.py:677-681): (inputfile -- a name inside HOME_DIR
    resolved --, HOME_DIR).  records None: the input is a file or `inputseq`."""
    if HOME_DIR is None:
        HOME_DIR = DATA_DIR
    if inputfile != None and not os.path.exists(inputfile) and os.path.exists(os.path.join(HOME_DIR, inputfile)):
        inputfile = os.path.join(HOME_DIR, inputfile)
    assert records is not None or os.path.exists(str(inputfile)) or inputseq, "Input file does not exist."
    assert fileformat in {'unknown', 'fasta', 'default', 'stockholm', 'clustal'}, \
        "Wrong fileformat, choose one of these: default,fasta,stockholm,clustal"
    return inputfile, HOME_DIR


def check_sources(records, inputfile, inputseq, fileformat, configfile, inputformat, HOME_DIR, priority):
    """check_input and Predict's checks of where the configuration comes from and of the input format, same messages
    (SQUARNA.py:677-703): (inputfile, configfile, whether the caller named one, priority names, HOME_DIR)."""
    inputfile, HOME_DIR = check_input(records, inputfile, inputseq, fileformat, HOME_DIR)
    configfile, configfileset, priority = find_config(configfile, HOME_DIR, priority)
    assert ''.join(sorted(inputformat.replace('x', ''))) in {"q", "fq", "qr", "qt", "qrt", "fqr", "fqt", "fqrt"}, \
        'Inappropriate inputformat value (subset of "fqrtx" with "q" being mandatory): {}'.format(inputformat)
    return inputfile, configfile, configfileset, priority, HOME_DIR


def _as_int(value, what, check, label):
    try:
        value = int(float(value))
        assert check(value)
        return value
    except Exception:
        raise ValueError("Inappropriate {} value ({}): {}".format(what, label, value))


_NOT_A_FLOAT = {"M": "Inappropriate M value (float): {}", "B": "Inappropriate B value (float): {}"}


def as_float(value, what):
    try:
        return float(value)
    except Exception:
        raise ValueError(_NOT_A_FLOAT[what].format(value))


def _rank_keys(rankby):
    """(rankbydiff, the order of the three scores) of a validated rankby string: SQUARNA.py:810-820."""
    if "r" in rankby and "s" in rankby:
        return "d" in rankby, (0, 2, 1)
    return "d" in rankby, (2, 0, 1) if "r" in rankby else (1, 2, 0)


_OPTIONS = frozenset(("maxstemnum", "threads", "M", "B", "algorithms", "rankby", "outplim", "toplim", "conslim", "poollim",
                      "reactformat", "levellimit", "freqlimit", "step3"))


def prediction_options(**given):
    """The prediction keywords that were passed, validated in Predict's order with its exception types and messages
    (SQUARNA.py:705-820): a dict of their values -- ``maxstemnum`` and ``levellimit`` None when unset, ``threads`` clamped,
    ``outplim`` the ``toplim`` when unset, ``rankby`` the order of the three scores -- plus ``algos`` with ``algorithms`` and
    ``rankbydiff`` with ``rankby``.  A keyword that is not passed is neither checked nor returned."""
    unknown = set(given) - _OPTIONS
    if unknown:
        raise TypeError("prediction_options: no such keyword: {}".format(", ".join(sorted(unknown))))
    out = {}
    positive = (lambda x: x > 0, "positive integer")
    if "maxstemnum" in given:
        v = given["maxstemnum"]
        out["maxstemnum"] = _as_int(v, "maxstemnum", lambda x: x >= 0, "non-negative integer") if v is not None else None
    if "threads" in given:
        try:
            out["threads"] = min(max(1, int(float(given["threads"]))), os.cpu_count())
        except Exception:
            raise ValueError("Inappropriate threads value (integer): {}".format(given["threads"]))
    for key in ("M", "B"):
        if key in given:
            out[key] = as_float(given[key], key)
    if "algorithms" in given:
        algorithms = out["algorithms"] = given["algorithms"]
        try:
            out["algos"] = set(algorithms.upper())
            assert out["algos"] <= {'E', 'G', 'H', 'N'}
        except Exception:
            raise ValueError('Inappropriate algorithm value (should be subset of "eghn"): {}'.format(algorithms))
    if "rankby" in given:
        rankby = given["rankby"]
        assert rankby in {"r", "s", "rs", "dr", "ds", "drs"}, \
            'Inappropriate rankby value (r/s/rs/dr/ds/drs): {}'.format(rankby)
        out["rankbydiff"], out["rankby"] = _rank_keys(rankby)
    if given.get("outplim") is not None:
        out["outplim"] = _as_int(given["outplim"], "outplim", *positive)
    if "toplim" in given:
        out["toplim"] = _as_int(given["toplim"], "toplim", *positive)
        if "outplim" in given and given["outplim"] is None:
            out["outplim"] = out["toplim"]
    for key in ("conslim", "poollim"):
        if key in given:
            out[key] = _as_int(given[key], key, *positive)
    if "reactformat" in given:
        reactformat = given["reactformat"]
        assert int(float(reactformat)) in {3, 10, 26}, "Inappropriate reactformat value (3/10/26): {}".format(reactformat)
        out["reactformat"] = int(float(reactformat))
    if "levellimit" in given:
        levellimit = out["levellimit"] = given["levellimit"]
        if levellimit is not None:
            try:
                out["levellimit"] = int(float(levellimit))
            except Exception:
                raise ValueError("Inappropriate levellimit value (integer): {}".format(levellimit))
    if "freqlimit" in given:
        out["freqlimit"] = as_freqlimit(given["freqlimit"])
    if "step3" in given:
        step3 = given["step3"]
        try:
            step3 = out["step3"] = step3.lower()
            assert step3 in {'u', 'i', '1', '2'}
        except Exception:
            raise _bad_freqlimit(step3)                              # (the reference's text for a bad step3, SQUARNA.py:806-808)
    return out


def _bad_freqlimit(freqlimit):
    return ValueError("Inappropriate freqlimit value (float between 0.0 and 1.0): {}".format(freqlimit))


def as_freqlimit(freqlimit):
    try:
        freqlimit = float(freqlimit)
        assert 0 <= freqlimit <= 1
        return freqlimit
    except Exception:
        raise _bad_freqlimit(freqlimit)


def alignment_defaults(defR, defS, defF, N, M, B):
    """Alignment mode's checks of the default reactivity, restraint and reference lines of an alignment of N columns
    (SQUARNA.py:944-958): the processed reactivities."""
    try:
        if defR:
            if len(defR) != N:
                defR = ProcessReacts(list(map(float, defR.split())), M=M, B=B)
            else:
                defR = ProcessReacts([ReactDict[ch] for ch in defR], M=M, B=B)
        assert not defR or len(defR) == N
    except Exception:
        raise ValueError('Inappropriate default reactivities line:\n {}'.format(defR))
    assert not defS or len(defS) == N, 'Inappropriate default restraints line:\n {}'.format(defS)
    assert not defF or len(defF) == N, 'Inappropriate default reference line:\n {}'.format(defF)
    return defR


def configs_by_length(configfile, configfileset, HOME_DIR, maxstemnum=None):
    """config_for(sequence) -> (paramset names, paramsets): the named configuration, or by length def / 500 / 1000
    (autoconfig, SQUARNA.py:868-878); maxstemnum overrides every paramset's."""
    configs = [ParseConfig(configfile)]
    if not configfileset:
        configs += [ParseConfig(os.path.join(HOME_DIR, "500.conf")), ParseConfig(os.path.join(HOME_DIR, "1000.conf"))]
    if maxstemnum is not None:
        for _, group in configs:
            for ps in group:
                ps['maxstemnum'] = maxstemnum

    def config_for(sequence):
        if configfileset or len(sequence) < 500:
            return configs[0]
        return configs[2] if len(sequence) >= 1000 else configs[1]
    return config_for


def batches(items, cells_of, max_records, max_cells):
    """The items in input order, cut into lists for one GPU batch each: a list ends with the item that brings it to
    max_records items or to max_cells cells (the sum of cells_of(item))."""
    batch, cells = [], 0
    for item in items:
        batch.append(item)
        cells += cells_of(item)
        if len(batch) >= max_records or cells >= max_cells:
            yield batch
            batch, cells = [], 0
    if batch:
        yield batch


def input_records(records, inputseq, inputfile, inputformat, fileformat, ignorewarn, inputrestr, M, B):
    """The (name, sequence, reactivities, restraints, reference) tuples of `records` or of the parsed input."""
    if records is not None:
        inputs = [(">record{}".format(k + 1), rec, None, None, None) if isinstance(rec, str) else tuple(rec)
                  for k, rec in enumerate(records)]
        assert all(len(rec) == 5 for rec in inputs), "records: sequences or (name, sequence, reactivities, restraints, reference)"
    else:
        with contextlib.redirect_stdout(io.StringIO()):          # (the parser announces a guessed file format)
            inputs = list(ParseInput(inputseq, inputfile, inputformat, fmt=fileformat, ignore=ignorewarn,
                                     inputrestr=inputrestr, M=M, B=B)[0])
    assert inputs, "No input records."
    return inputs


def derived_inputs(entry, records, inputfile, inputseq, inputformat, fileformat, ignorewarn, M, B, fold_keywords):
    """The opening of an entry that builds its own records and calls ``Fold`` (FoldWindows, FoldMutants, a side of
    FoldDuplex): the input's synonyms picked out of `fold_keywords`, ``bpp`` refused, M and B converted, the sources
    checked.  Returns (the parsed input records, the keywords for ``Fold(records=..., **keywords)``)."""
    kw = dict(fold_keywords)
    inputfile = pick(inputfile, kw.pop("i", None)); inputseq = pick(inputseq, kw.pop("seq", None), kw.pop("s", None))
    fileformat = pick(fileformat, kw.pop("ff", None)); ignorewarn = pick(ignorewarn, kw.pop("ignore", None), kw.pop("iw", None))
    if kw.get("bpp") is not None:
        raise ValueError("{} does not cover bpp: use Fold".format(entry))
    M, B = as_float(M, "M"), as_float(B, "B")
    inputfile = check_sources(records, inputfile, inputseq, fileformat, kw.get("configfile"), inputformat,
                              kw.get("HOME_DIR"), kw.get("priority"))[0]
    inputs = input_records(records, inputseq, inputfile, inputformat, fileformat, ignorewarn, kw.pop("inputrestr", None), M, B)
    return inputs, dict(kw, inputformat=inputformat, ignorewarn=ignorewarn, M=M, B=B)
