"""GPU tests of the g4 / rbp options: Predict on the HIP engine prints the reference's text byte for byte (the found
restraints -- long '+' runs, a forced Fab pair -- go through the fill and scan kernels' restraint flags), and
PredictSharded under a world-1 RCCL group equals Predict."""
import hashlib
import io
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(GOLDEN))

with open(os.path.join(GOLDEN, "motifs.json")) as f:
    TEXTS = json.load(f)["texts"]
# (the default configuration folds with ViennaRNA's base-pair probabilities: its text is checked on the CPU, on the
# stand-in tests/fake_rna.py)
GPU_TEXTS = sorted(t for t, d in TEXTS.items() if "configfile" in d["args"] or d["args"].get("alignment"))


def _args(tag):
    kw = dict(TEXTS[tag]["args"])
    if "inputfile" in kw:
        kw["inputfile"] = os.path.join(ROOT, kw["inputfile"])
    return kw


def _expected(tag):
    with open(os.path.join(GOLDEN, "text", tag + ".txt")) as f:
        return f.read()


@pytest.mark.gpu
@pytest.mark.parametrize("tag", GPU_TEXTS)
def test_motif_text_matches_reference_on_gpu(tag, capsys):
    from squarna_amd import Predict
    buf = io.StringIO()
    Predict(write_to=buf, **_args(tag))
    txt, exp = buf.getvalue(), _expected(tag)
    if txt != exp:
        tl, el = txt.split("\n"), exp.split("\n")
        bad = [(k, a, b) for k, (a, b) in enumerate(zip(tl, el)) if a != b][:3]
        raise AssertionError("text differs (%d vs %d lines): %r" % (len(tl), len(el), bad))
    assert hashlib.sha256(txt.encode()).hexdigest() == TEXTS[tag]["sha256"]
    assert capsys.readouterr().err == TEXTS[tag]["stderr"]


@pytest.mark.gpu
def test_predict_sharded_g4_under_nccl_world1(tmp_path, capsys):
    """One input record: PredictSharded's output equals Predict's, with the search run (and a warning printed) once."""
    import torch
    import torch.distributed as dist
    from squarna_amd.parallel import PredictSharded
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    assert not dist.is_initialized()
    dist.init_process_group("nccl", init_method="file://" + str(tmp_path / "rdzv"), rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    try:
        for tag in ("motif_readme_g4_nobpp", "motif_default_qtrf_g4rbp_nobpp", "motif_two_records_g4_nobpp"):
            buf = io.StringIO()
            PredictSharded(write_to=buf, **_args(tag))
            assert buf.getvalue() == _expected(tag), tag
            warning = "WARNING: Found more than one sequence, rfam/G4/RBP search disabled.\n"
            assert capsys.readouterr().err.count(warning) == TEXTS[tag]["stderr"].count(warning), tag
    finally:
        dist.destroy_process_group()
