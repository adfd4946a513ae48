"""What the five tool benches (scripts/{verify,coverage,linkage,align,draft}_bench.py)
share: the common arguments, the package and its device scope (or the exit
without a GPU), the HIP-event timing and the JSON lines."""
import importlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def parse(ap, repeats, warmup):
    """The parsed arguments: the bench's own (already added to ``ap``) and the
    shared ones, with the bench's defaults."""
    ap.add_argument("--repeats", type=int, default=repeats)
    ap.add_argument("--warmup", type=int, default=warmup)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out")
    return ap.parse_args()


def gpu(device):
    """(package, its scope of a call on GPU ``device``); exits without a GPU."""
    pkg = importlib.import_module("minion-plasmid-consensus_amd")
    pkg.engine.lib()
    import torch
    if not torch.cuda.is_available():
        sys.exit("%s measures on a GPU; none is visible" % os.path.basename(sys.argv[0]))
    return pkg, importlib.import_module(pkg.__name__ + "._native").Device(device)


def timed(d, launch, warmup, repeats):
    """[ms] of ``repeats`` runs of launch(), each between two HIP events on the
    scope's current stream, after ``warmup`` untimed runs."""
    torch = d.torch
    stream = torch.cuda.current_stream(d.dev)
    for _ in range(warmup):
        launch()
    torch.cuda.synchronize(d.dev)
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        launch()
        e1.record(stream)
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return times


def report(results, rec):
    print(json.dumps(rec), flush=True)
    results.append(rec)


def write(results, out):
    if out:
        with open(out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
