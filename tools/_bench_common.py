"""What tools/bench_predict.py, bench_fullres.py and bench_ensemble.py share: the event timer, the
peak-memory probe, the per-variant statistics and the writing of the JSON report."""
import json
import os
import statistics

import torch

HBM_PEAK = 8.0e12                                                     # bytes / s


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters                      # us per call


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return peak


def spread(v, digits=1, prefix="us_"):
    """Median, min and max of the rounds' samples."""
    return {prefix + "median": round(statistics.median(v), digits), prefix + "min": round(min(v), digits),
            prefix + "max": round(max(v), digits)}


def variant_rows(samples, bytes_moved, peaks):
    """Per variant: the spread, the algorithmic bytes over the median as a share of the HBM peak, peak memory."""
    rows = {}
    for k, v in samples.items():
        rows[k] = dict(spread(v), algorithmic_bytes=bytes_moved[k],
                       share_of_hbm_peak=round(bytes_moved[k] / (statistics.median(v) * 1e-6) / HBM_PEAK, 4),
                       peak_memory_bytes=peaks[k])
    return rows


def write_report(report, out):
    """One JSON line on stdout and, with ``out``, the indented report in that file."""
    print(json.dumps(report))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")
