"""The front the command-line tools share: status lines, the drop-ins' banner,
finding the package, the argparse types, and the tail of a report tool's main
(error line, output files, verdict, exit status).

Standard library only, and nothing of the package is imported here: --help and
an argparse error need no native library.  A tool finds this module with

    if __package__:
        from . import _cli
    else:  # run by path: sys.path[0] is this directory
        import _cli

(the directory name is not an identifier, so a file run by path cannot name the
package in an import statement).
"""
import argparse
import importlib
import os
import sys
import time

_RULE = "======================================================="


def statprint(msg, msg_type="STATUS", colour=False):
    """'STATUS [time]: msg' on stdout; colour: the reference's escape codes (pseudopair_reads)."""
    form = "\033[1;37;40m{}\033[0m \033[1;34;40m[{}]\033[0m: {}" if colour else "{} [{}]: {}"
    print(form.format(msg_type, time.strftime("%Y/%m/%d %T"), msg), flush=True)


def banner(extra=()):
    """The reference scripts' opening block; extra: lines of ours before the closing rule."""
    print(_RULE)
    print("Python version: {}".format(sys.version))
    print("Python environment: {}".format(sys.prefix))
    print("Server: {}".format(os.uname()[1]))
    print("Current directory: {}".format(os.getcwd()))
    print("Command: {}".format(" ".join(sys.argv)))
    print("Time: {}".format(time.strftime("%Y/%m/%d %T")))
    for line in extra:
        print(line)
    print(_RULE + "\n")


def package(file, package_name):
    """The package of the tool `file`, whose __package__ is package_name: imported
    by that name, or (run by path) by its directory's name from the directory above."""
    if package_name:
        return importlib.import_module(package_name)
    here = os.path.dirname(os.path.abspath(file))
    sys.path.insert(0, os.path.dirname(here))
    return importlib.import_module(os.path.basename(here))


def device_arg(text):
    if text == "cpu":
        return text
    try:
        return int(text)
    except ValueError:
        raise argparse.ArgumentTypeError("a HIP device index or 'cpu'")


def gpu_arg(text):
    """--device of a tool with no host path."""
    try:
        return int(text)
    except ValueError:
        raise argparse.ArgumentTypeError("a HIP device index (there is no 'cpu': the pileup has no host path)")


def fraction_arg(text):
    """--max-error: a number >= 0."""
    try:
        v = float(text)
    except ValueError:
        v = -1.0
    if not v >= 0:
        raise argparse.ArgumentTypeError("a number >= 0")
    return v


def region_arg(text):
    try:
        lo, hi = (int(x) for x in text.split(":"))
    except ValueError:
        raise argparse.ArgumentTypeError("START:END (0-based, half-open)")
    return lo, hi


def place(device):
    return "the host" if device == "cpu" else "device {}".format(device)


def fail(e):
    """'Error: e' on stderr; the exit status 1."""
    print("Error: {}".format(e), file=sys.stderr)
    return 1


def write_texts(outputs):
    """Writes [(path, text)] in order: 0, or fail() at the first path that
    cannot be written (the files before it stay)."""
    try:
        for path, text in outputs:
            with open(path, "w") as f:
                f.write(text)
    except OSError as e:
        return fail(e)
    return 0


def verdict_exit(label, strict, verdict):
    """The last two status lines of a report tool; its exit status: 2 on FAIL with --strict, else 0."""
    statprint("{}: {}".format(label, verdict))
    statprint("Done.")
    return 2 if strict and verdict == "FAIL" else 0


def key_value_report(keys, rows_of_values, verdict, verdict_key="verdict"):
    """One 'key<TAB>value' line per key for every row of values, then the verdict line."""
    out = ["{}\t{}\n".format(k, v) for values in rows_of_values for k, v in zip(keys, values)]
    out.append("{}\t{}\n".format(verdict_key, verdict))
    return "".join(out)
