"""Writes profiles/stream_geometry.txt: per case of tests/stream_geometry.py and quantity group the mirror's own spread under one-ulp input noise, the
deviation of the CPU build of the kernel text from the mirror and -- with --gpu, on a machine with one -- the device's, all as the worst |a - b| / (1 + |b|)
over the case's ticks ("update": absolute, table and state behind the re-plan against apply_update).  The tests recompute what they need and write nothing.

    python -m tests.stream_geometry_profile [--gpu] [output file]
"""
import contextlib
import io
import os
import sys

from tests import stream_geometry as sg


def main(argv):
    gpu = "--gpu" in argv
    rest = [a for a in argv if a != "--gpu"]
    out = rest[0] if rest else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "stream_geometry.txt")
    quiet = contextlib.redirect_stdout(io.StringIO())      # (the mirror prints the reference's warnings)
    with quiet:
        cpu = {n: sg.cpu_run(n) for n in sg.names()}
        spread = {n: sg.spread_of(n) for n in sg.names()}
        dev = {}
        if gpu:
            shapes = sorted(set(sg.shapes("replay") + sg.shapes("replan")))
            for N, S in shapes:
                dev.update(sg.gpu_run(sg.names("replay", (N, S)) + sg.names("replan", (N, S)), update=True))
            dev.update(sg.gpu_run(sg.names("sweep")))
    fmt = lambda v: "        -" if v is None else f"{v:9.2e}"
    lines = ["# stream kernels against the host mirror on random paths (tests/stream_geometry.py; written by tests/stream_geometry_profile.py)",
             "# worst |a - b| / (1 + |b|) over the ticks of a case; bound: the fixed bound of the group, or 100 x spread where the case takes it from the mirror",
             f"# {'case':<22} {'group':<7} {'spread':>9} {'cpu build':>9} {'device':>9} {'bound':>9}"]
    worst = {}
    for n in sg.names():
        tol = sg.tolerances(n)
        for g in list(sg.GROUPS) + ["update"]:
            if g not in cpu[n]:
                continue
            row = (spread[n].get(g), cpu[n][g][0], dev[n][g][0] if n in dev and g in dev[n] else None)
            lines.append(f"  {n:<22} {g:<7} {fmt(row[0])} {fmt(row[1])} {fmt(row[2])} {fmt(tol[g])}")
            w = worst.setdefault(g, [0.0, 0.0, 0.0])
            for i, v in enumerate(row):
                if v is not None and not sg.BY_NAME[n]["spread"]:
                    w[i] = max(w[i], v)
    lines.append("# worst over the cases on the fixed bound")
    for g, w in worst.items():
        lines.append(f"  {'all':<22} {g:<7} {fmt(w[0])} {fmt(w[1])} {fmt(w[2] if gpu else None)} {fmt(sg.TOL[g])}")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {out}: {len(lines)} lines")


if __name__ == "__main__":
    main(sys.argv[1:])
