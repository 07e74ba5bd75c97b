"""Every SQ_* environment variable the Python layer reads, one function each (the library's are in csrc/sq_switches.h;
INTEGRATION.md section 5 documents both).  Each call reads the environment anew: tests flip them between two folds of one
process.  A presence switch is on whenever the variable is set, whatever its value."""
import os


def no_pool_kept():
    """SQ_NO_POOL_KEPT (presence): no kept-list pages in the slot estimate, as the library reserves none."""
    return "SQ_NO_POOL_KEPT" in os.environ


def kept_pps():
    """SQ_KEPT_PPS=<pages>: kept-list pages per structure slot and generation in the slot estimate; None: the default."""
    return float(os.environ["SQ_KEPT_PPS"]) if "SQ_KEPT_PPS" in os.environ else None


def mul_gather():
    """SQ_MUL_GATHER (presence): an alignment's rows get gathered N x N slices, which bound a sub-batch as dense matrices."""
    return "SQ_MUL_GATHER" in os.environ


def dense_gb():
    """SQ_DENSE_GB=<GB>: dense per-job matrices one sub-batch of fold_records may hold (default 32)."""
    return float(os.environ.get("SQ_DENSE_GB", "32"))


def engine_sublanes():
    """SQ_ENGINE_SUBLANES=k: sub-batches of a wide-pool input folded k at a time from threads (default 1, at least 1)."""
    return max(1, int(os.environ.get("SQ_ENGINE_SUBLANES", "1")))


def engine_lanes():
    """SQ_ENGINE_LANES=k: k >= 2 cuts one big fold_records call into two concurrent batches (default 1)."""
    return int(os.environ.get("SQ_ENGINE_LANES", "1"))


def no_detach():
    """SQ_NO_DETACH (presence): fold_records_packed copies the records out of the library's pinned buffer."""
    return "SQ_NO_DETACH" in os.environ


def no_packed_rows():
    """SQ_NO_PACKED_ROWS (presence): alignment step 1 prepares its rows one Prepared record at a time."""
    return "SQ_NO_PACKED_ROWS" in os.environ
