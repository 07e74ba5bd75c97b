"""``Predict`` and ``Main``: the drop-in API/CLI surface of SQUARNA (SQUARNA.py:416-1257).

Same keyword arguments, synonyms, validation messages, config lookup and output text as the
reference.  Single-sequence predictions are batched across the input records and folded on
the GPU (the reference parallelises the same loop over CPU processes, SQUARNA.py:887-935);
blocks are printed in input order; alignment mode (``a``) runs through ``squarna_amd.align``.
``bpp != 0`` paramsets take their base-pair probabilities from ViennaRNA on the host (``import RNA``,
as the reference does).  ``g4`` / ``rbp`` restraint discovery for a single input record runs on the host
(``squarna_amd.motifs``).  Out of scope of this build: Rfam restraint discovery (``rfam``).
"""
import io
import os
import sys

from .config import DATA_DIR
from .dbn import GAPS
from .inputs import ParseInput
from .options import alignment_defaults, batches, check_sources, configs_by_length, pick, prediction_options
from .core import RunSQRNdbnseq, resolve_priority
from . import engine as _engine

#: records folded per GPU batch (bounded by the sum of N^2 as well)
BATCH_RECORDS = 16384                 # records folded in one GPU batch (bigger batches: fewer, fuller kernel launches)
BATCH_CELLS = 2 * 1024 * 1024 * 1024   # ... bounded by sum of N^2 x paramsets


def Predict(inputfile=None, fileformat="unknown", inputseq=None, configfile=None, inputformat="qtrf",
            maxstemnum=None, threads=os.cpu_count(), byseq=False, algorithms='', entropy=False,
            rankby="r", evalonly=False, hardrest=False, interchainonly=False, toplim=5, outplim=None,
            conslim=1, poollim=1000, reactformat=3, alignment=False, levellimit=None, freqlimit=0.35,
            verbose=False, step3="u", ignorewarn=False, HOME_DIR=None, write_to=None, priority=None,
            rfam=False, g4=False, M=1.8, B=-0.6, rbp=False,
            i=None, ff=None, c=None, config=None, s=None, seq=None, a=None, ali=None, algo=None,
            algorithm=None, rb=None, fl=None, freqlim=None, ll=None, levlim=None, tl=None, ol=None,
            cl=None, pl=None, pr=None, s3=None, msn=None, rf=None, eo=None, hr=None, ico=None, iw=None,
            ignore=None, t=None, bs=None, v=None, inputrestr=None, _select=None, _on_block=None,
            _lengths_only=False):
    """Print SQUARNA predictions for the given input (see SQUARNA.py:431-600 for the
    meaning of every parameter; short synonyms are accepted exactly as there)."""
    # synonyms, later ones win as in SQUARNA.py:602-664
    inputfile = pick(inputfile, i); fileformat = pick(fileformat, ff)
    configfile = pick(configfile, config, c); inputseq = pick(inputseq, seq, s)
    alignment = pick(alignment, ali, a); algorithms = pick(algorithms, algorithm, algo)
    rankby = pick(rankby, rb); freqlimit = pick(freqlimit, freqlim, fl)
    levellimit = pick(levellimit, levlim, ll); toplim = pick(toplim, tl); outplim = pick(outplim, ol)
    conslim = pick(conslim, cl); poollim = pick(poollim, pl); priority = pick(priority, pr)
    step3 = pick(step3, s3); maxstemnum = pick(maxstemnum, msn); reactformat = pick(reactformat, rf)
    evalonly = pick(evalonly, eo); hardrest = pick(hardrest, hr); interchainonly = pick(interchainonly, ico)
    ignorewarn = pick(ignorewarn, ignore, iw); threads = pick(threads, t); byseq = pick(byseq, bs)
    verbose = pick(verbose, v)
    if write_to is None:
        write_to = sys.stdout

    # ---- validation (SQUARNA.py:677-820), same messages: options.py
    inputfile, configfile, configfileset, priority, HOME_DIR = check_sources(None, inputfile, inputseq, fileformat, configfile,
                                                                             inputformat, HOME_DIR, priority)
    opt = prediction_options(maxstemnum=maxstemnum, threads=threads, M=M, B=B, algorithms=algorithms, rankby=rankby,
                             outplim=outplim, toplim=toplim, conslim=conslim, poollim=poollim, reactformat=reactformat,
                             levellimit=levellimit, freqlimit=freqlimit, step3=step3)
    threads, M, B, algos, rankbydiff, rankby = (opt[k] for k in ("threads", "M", "B", "algos", "rankbydiff", "rankby"))
    outplim, toplim, conslim, poollim, reactformat = (opt[k] for k in ("outplim", "toplim", "conslim", "poollim", "reactformat"))
    levellimit, freqlimit, step3 = opt["levellimit"], opt["freqlimit"], opt["step3"]

    if alignment and not configfileset:                          # SQUARNA.py:822-824
        configfile = os.path.join(HOME_DIR, "ali.conf")
    if rfam:
        raise NotImplementedError("Rfam restraint discovery (Infernal's cmscan, SQRNrfam.py) is out of scope of this build")

    config_for = configs_by_length(configfile, configfileset, HOME_DIR, opt["maxstemnum"])   # autoconfig, SQUARNA.py:868-878

    inputs, fmt, single_input = ParseInput(inputseq, inputfile, inputformat, fmt=fileformat,
                                           ignore=ignorewarn, inputrestr=inputrestr, M=M, B=B)
    if _lengths_only:                                            # PredictSharded: the cost model's record lengths
        return [len(rec[1]) for rec in inputs]
    if alignment:                                                # SQUARNA.py:938-991
        from .align import RunSQRNdbnali
        defR, defS, defF = ParseInput(inputseq, inputfile, inputformat, returndefaults=True, fmt=fmt,
                                      ignore=ignorewarn, M=M, B=B)[0]
        objs = [obj for obj in inputs]
        N = len(objs[0][1])
        assert all(len(obj[1]) == N for obj in objs), 'The sequences are not aligned'
        defR = alignment_defaults(defR, defS, defF, N, M, B)
        if levellimit is None:
            levellimit = 3 - int(N > 500)
        paramsetnames, paramsets = config_for("")                # (ali.conf or the named configuration: not chosen by length)
        RunSQRNdbnali(objs, defR, defS, defF, levellimit, freqlimit, verbose, step3, paramsetnames, paramsets,
                      threads, rankbydiff, rankby, hardrest, interchainonly, toplim, outplim, conslim, reactformat,
                      poollim, entropy=entropy, algos=algos, sink=write_to, M=M, B=B)
        return
    rfamlabel = False                                            # SQUARNA.py:850-866: G4 / RBP restraints, one record only
    if g4 or rbp:
        if not single_input:
            print("WARNING: Found more than one sequence, rfam/G4/RBP search disabled.", file=sys.stderr)
        elif _select is None or 0 in _select:
            from .motifs import SearchG4RBP
            inputs = [list(rec) for rec in inputs]
            found, rfamlabel = SearchG4RBP(inputs[0][1], g4, rbp)
            if found:
                inputs[0][3] = found                             # (replaces any restraint line of the input)

    eng = _engine.get_engine()
    common = dict(conslim=conslim, toplim=toplim, hardrest=hardrest, rankbydiff=rankbydiff, rankby=rankby,
                  interchainonly=interchainonly, poollim=poollim, algos=algos, levellimit=levellimit, M=M, B=B,
                  keep=max(int(outplim), 1))                     # (only the printed structures are fetched)

    def flush(batch):
        """Fold a batch of records on the GPU, then print every block in input order."""
        preds = [None] * len(batch)
        refsc = [None] * len(batch)
        texts = [None] * len(batch)
        if not evalonly and not entropy:
            # records with different priority index sets cannot share one fold call
            groups = {}
            for k, rec in enumerate(batch):
                names = rec[5]
                groups.setdefault(tuple(sorted(resolve_priority(priority, names, rfamlabel))), []).append(k)
            # The library writes the output blocks itself (sq_write_blocks) when the engine can: the records then carry their
            # block fields (name, encoded reactivity line, which list of paramset names they print).  Not a record with G4 /
            # RBP restraints (rfamlabel: the only record of its input): its block carries the label and the '+' marks.
            blocks = getattr(eng, "writes_blocks", False) and not rfamlabel
            psnames, psname_idx = [], {}
            for prio, idx in groups.items():
                if blocks:
                    from .dbn import EncodedReactivities
                    recs = []
                    for k in idx:
                        name, seq, reacts, restrs, ref, names = batch[k][:6]
                        key = id(names)
                        if key not in psname_idx:
                            psname_idx[key] = len(psnames)
                            psnames.append(list(names))
                        rline = str(EncodedReactivities(seq, reacts, reactformat)) if reacts else None
                        recs.append((seq, reacts, restrs, ref, batch[k][6], None, name, rline, psname_idx[key]))
                    res = eng.fold_records(recs, priority=set(prio), _blocks=dict(psnames=psnames, conslim=conslim, outplim=outplim),
                                           **common)
                    if len(groups) == 1 and not _on_block and hasattr(res, "blocks") and hasattr(res.blocks, "text"):
                        write_to.write(res.blocks.text)            # every block of the batch, in input order: one write
                        return
                    for k, (kind, val) in zip(idx, res):
                        if kind == "text":
                            texts[k] = val
                        else:
                            preds[k], refsc[k] = val
                    continue
                res = eng.fold_records([(batch[k][1], batch[k][2], batch[k][3], batch[k][4], batch[k][6], None)
                                        for k in idx], priority=set(prio), **common)
                got_ref = getattr(eng, "last_ref_scores", None)
                for q, (k, r) in enumerate(zip(idx, res)):
                    preds[k] = r
                    if got_ref is not None and len(got_ref) == len(idx):
                        refsc[k] = got_ref[q]
        for k, (name, seq, reacts, restrs, ref, names, psets, index) in enumerate(batch):
            if texts[k] is not None:                               # the library's block: byte for byte RunSQRNdbnseq's
                if _on_block:
                    _on_block(index, texts[k])
                else:
                    write_to.write(texts[k])
                continue
            sink = io.StringIO() if _on_block else write_to
            RunSQRNdbnseq(name, seq, reacts, restrs, ref, names, psets, threads, rankbydiff, rankby,
                          hardrest, interchainonly, toplim, outplim, conslim, reactformat, evalonly, poollim,
                          mp=False, sink=sink, entropy=entropy, algos=algos, levellimit=levellimit,
                          priority=priority, rfam=rfamlabel, M=M, B=B, _prediction=preds[k], _ref_scores=refsc[k])
            if _on_block:
                _on_block(index, sink.getvalue())

    # (thousands of small result containers: the cyclic collector only costs time here, see HipEngine.fold_records)
    import gc
    gc_was = gc.isenabled()
    gc.disable()
    try:
        _predict_records(inputs, _select, config_for, flush)
    finally:
        if gc_was:
            gc.enable()


def _predict_records(inputs, _select, config_for, flush):
    """The record loop of Predict's single-sequence mode: batches of records folded on the GPU, blocks printed in
    input order (the reference's ordered Pool.imap, SQUARNA.py:887-935)."""
    chosen = ((name, seq, reacts, restrs, ref) + config_for(seq) + (index,)
              for index, (name, seq, reacts, restrs, ref) in enumerate(inputs) if _select is None or index in _select)
    for batch in batches(chosen, lambda rec: len(rec[1]) * len(rec[1]) * len(rec[6]), BATCH_RECORDS, BATCH_CELLS):
        flush(batch)


def Main():
    """Command line: ``key=value`` tokens, bare flags and ``-key value`` forms (SQUARNA.py:994-1257)."""
    def usage():
        print("\nUsage:\n\nSQUARNA i=inputfile [OPTIONS]\n\nSQUARNA s=ACGUGUCAC [OPTIONS]\n")
        print("For further details read the help message:\n\nSQUARNA --help\n")
        sys.exit(1)

    args = sys.argv[1:]
    if not args:
        usage()
    if any(h in args for h in ("--help", "-help", "help", "--h", "-h", "h", "--H", "-H", "H")):
        readme = os.path.join(DATA_DIR, "README.md")
        print(open(readme).read() if os.path.exists(readme) else Predict.__doc__)
        sys.exit(0)

    valued = {"algo", "algorithm", "algos", "algorithms", "b", "c", "config", "i", "input", "if", "inputformat",
              "rb", "rankby", "ff", "fileformat", "fl", "freqlim", "ll", "levlim", "tl", "toplim", "ol",
              "outplim", "cl", "conslim", "pl", "poollim", "pr", "priority", "s3", "step3", "m", "msn",
              "maxstemnum", "rf", "reactformat", "s", "seq", "sequence", "t", "threads"}
    flags = {"a", "ali", "alignment", "bs", "byseq", "ent", "entropy", "eo", "evalonly", "g4", "hr", "hardrest",
             "iw", "ignore", "ico", "interchainonly", "rbp", "rfam", "v", "verbose"}
    norm, k = [], 0
    while k < len(args):                                         # "-key value" -> "key=value"
        tok = args[k]
        bare = tok.lstrip('-').lower()
        if tok.startswith('-') and tok.count('-') <= 2 and bare in valued and len(tok) - len(tok.lstrip('-')) in (1, 2):
            norm.append(tok.lstrip('-') + '=' + args[k + 1])
            k += 1
        elif tok.startswith('-') and bare in flags and len(tok) - len(tok.lstrip('-')) in (1, 2):
            norm.append(tok.lstrip('-'))
        else:
            norm.append(tok)
        k += 1

    kw = dict(poollim=100)                                       # CLI default differs from the API (SQUARNA.py:1047)
    keymap = {"algo": "algorithms", "algos": "algorithms", "algorithm": "algorithms", "algorithms": "algorithms",
              "s": "inputseq", "seq": "inputseq", "sequence": "inputseq", "i": "inputfile", "input": "inputfile",
              "ff": "fileformat", "fileformat": "fileformat", "c": "configfile", "config": "configfile",
              "if": "inputformat", "inputformat": "inputformat", "msn": "maxstemnum", "maxstemnum": "maxstemnum",
              "t": "threads", "threads": "threads", "rb": "rankby", "rankby": "rankby", "tl": "toplim",
              "toplim": "toplim", "ol": "outplim", "outplim": "outplim", "cl": "conslim", "conslim": "conslim",
              "pl": "poollim", "poollim": "poollim", "pr": "priority", "priority": "priority",
              "rf": "reactformat", "reactformat": "reactformat", "ll": "levellimit", "levlim": "levellimit",
              "levellim": "levellimit", "levlimit": "levellimit", "levellimit": "levellimit", "fl": "freqlimit",
              "freqlim": "freqlimit", "freqlimit": "freqlimit", "frequencylim": "freqlimit",
              "frequencylimit": "freqlimit", "s3": "step3", "step3": "step3", "m": "M", "b": "B"}
    flagmap = {"bs": "byseq", "byseq": "byseq", "eo": "evalonly", "evalonly": "evalonly", "hr": "hardrest",
               "hardrest": "hardrest", "ico": "interchainonly", "interchainonly": "interchainonly",
               "a": "alignment", "ali": "alignment", "alignment": "alignment", "v": "verbose",
               "verbose": "verbose", "iw": "ignorewarn", "ignore": "ignorewarn", "ent": "entropy",
               "entropy": "entropy", "rbp": "rbp", "rfam": "rfam", "g4": "g4"}
    lowered = {"fileformat", "inputformat"}
    for arg in norm:
        key, eq, val = arg.partition('=')
        lk = key.lower()
        if eq and lk in keymap:
            dest = keymap[lk]
            if dest == "algorithms" and not val:
                continue
            if dest in lowered:
                val = val.lower()
            if dest == "rankby":
                val = ''.join(sorted(val.lower()))
            kw[dest] = val
        elif not eq and lk in flagmap:
            kw[flagmap[lk]] = True
        elif len(norm) == 1:                                     # a lone token: file or sequence
            if os.path.exists(arg):
                kw["inputfile"] = arg
            elif sum(arg.lower().count(x) for x in (GAPS | set("acgut"))) > len(arg) / 2:
                kw["inputseq"] = arg
            else:
                kw["inputfile"] = arg
        else:
            print("Unrecognized option: {}".format(arg))
    print(kw.get("inputfile"))                                   # SQUARNA.py:1248
    Predict(**kw)


if __name__ == "__main__":
    Main()
