#!/usr/bin/env python3
"""Round-6 experiment variants of libmpc.so: named text substitutions of the
product source (timing / counter variants; ablations give wrong results and are
never shipped).  Writes exp/v/src/<name>.hip (git-ignored) and builds
exp/v/<name>.so:   python3 exp/r06/variants.py name [name ...]   (or: all)"""
import os
import subprocess
import sys

R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SRC = os.path.join(R, "minion-plasmid-consensus_amd/csrc/mpc_kernels.hip")

S1_STORE = "        if (sev) a.subev[sev_base + nsub_s + lanes_below(bw)] = ev;"
WIN_STORE = "          if (mine) wp[n0 + lanes_below(bw)] = (uint16_t)(((uint32_t)(i & (kSubWin - 1)) << 2) | pay);"
PG_STORE = "  if (fast) pg0[(old >> kPgBits) * kPgEv + (old & ((1u << kPgBits) - 1u))] = word;"
FAST = ("        fast = !v | (!lfar & ((olen >= 1) & (olen <= 4) & dig &\n"
        "                              (colon | minus | (star & (((bad >> shl) & 0xffu) == 0u)) | (plus & ((bad & vm) == 0u))) |\n"
        "                              nop));")

# (the lean / lazy / speculative / split variants of this round patched switches
# that commit b26663d holds and the product no longer does: build them from
# that commit's source.  The variants that flipped a compile-time switch --
# intcheck_all, intcheck_old, defersub, interp, leftdiag, flushx2, nodefer,
# prefetch, m12opt -- need the source of commit a668828, the last one that
# holds those switches: DESIGN.md section 7, dropped variants)
VARIANTS = {
    "base": [],
    # counters: which store stream carries C5's write amplification
    "noevstore": [(PG_STORE, "")],
    "nosubstore": [(S1_STORE, ""), (WIN_STORE, "")],
    "subnt": [
        (S1_STORE, "        if (sev) __builtin_nontemporal_store(ev, a.subev + sev_base + nsub_s + lanes_below(bw));"),
        (WIN_STORE, "          if (mine) __builtin_nontemporal_store((uint16_t)(((uint32_t)(i & (kSubWin - 1)) << 2) | pay), "
                    "wp + n0 + lanes_below(bw));"),
    ],
    "noflush": [("      if (dv) atomicAdd(a.diff + gb + p, dv);", "      (void)dv;"),
                ("      if (v) atomicAdd(sg + k, v);", "      (void)v; (void)sg;")],
    "leftnosearch": [("      if (lb > la) {", "      if (lb < 0 && lb > la) {")],
    "leftnotally": [("          if (j < L) atomicAdd(tp + 4 * (L - 1 - j) + (int)((ev >> (2 * j)) & 3u), 1u);",
                     "          if (j < L && ev == 0x7fffffffu) atomicAdd(tp + 4 * (L - 1 - j) + (int)((ev >> (2 * j)) & 3u), 1u);")],
    # timing upper bound of dropping the per-unit canonical check: no check, no
    # general decode (right results only on canonical input)
    "nocheck": [(FAST, "        fast = true; (void)dig; (void)bad; (void)vm; (void)nop; (void)lfar;"),
                ("        if (ballot(!fast)) return false;  // (before any effect: the round restarts on the general decode)",
                 "")],
}


def build(name):
    s = open(SRC).read()
    for a, b in VARIANTS[name]:
        assert s.count(a) == 1, (name, a[:80])
        s = s.replace(a, b)
    d = os.path.join(R, "exp/v/src")
    os.makedirs(d, exist_ok=True)
    src = os.path.join(d, name + ".hip")
    open(src, "w").write(s)
    out = os.path.join(R, "exp/v", name + ".so")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
           "-I", os.path.join(R, "include"), "-I", os.path.join(R, "minion-plasmid-consensus_amd/csrc"), "-o", out, src]
    subprocess.run(cmd, check=True)
    print("built", out)


if __name__ == "__main__":
    names = list(VARIANTS) if sys.argv[1:] == ["all"] else sys.argv[1:]
    for n in names:
        build(n)
