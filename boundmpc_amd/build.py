"""Build the HIP extension in-tree: boundmpc_amd/csrc/libboundmpc_hip.so (gfx950 only)."""
import collections
import glob
import hashlib
import os
import re
import shlex
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(CSRC, "libboundmpc_hip.so")
ISA_DIR = os.path.join(HERE, "..", "build", "isa")      # <unit>.o, <unit>_gfx950.s (the device listing of the same compilation), <unit>.d
SOURCES = [os.path.join(CSRC, "bmpc_hip.hip"), os.path.join(CSRC, "bmpc_wave.inl"), os.path.join(CSRC, "bmpc_stream.inl"),
           os.path.join(HERE, "..", "include", "boundmpc_hip.h"), os.path.join(CSRC, "bmpc_team.hip"), os.path.join(CSRC, "bmpc_gpu_common.h"),
           os.path.join(CSRC, "bmpc_resto.hip"), os.path.join(CSRC, "bmpc_tick.hip"), os.path.join(CSRC, "bmpc_pair.hip"),
           os.path.join(CSRC, "bmpc_multi_batch.inl"), os.path.join(CSRC, "bmpc_tick_kernel.inl"), os.path.join(CSRC, "bmpc_dual.inl"), os.path.join(CSRC, "bmpc_kkt.inl"), os.path.join(CSRC, "bmpc_sens.inl"), os.path.join(CSRC, "bmpc_args.h"),
           os.path.join(CSRC, "bmpc_stream_log.inl"), os.path.join(CSRC, "bmpc_stream_update.inl"), os.path.join(CSRC, "bmpc_rollout.hip"),
           os.path.join(CSRC, "bmpc_rollout_kernel.inl"), os.path.join(CSRC, "bmpc_stream_events.inl"), os.path.join(CSRC, "bmpc_rollout_events.hip"),
           os.path.join(CSRC, "bmpc_stream_tube.inl"), os.path.join(CSRC, "bmpc_rollout_audit.hip"),
           os.path.join(CSRC, "bmpc_rollout_log.hip"), os.path.join(CSRC, "bmpc_team_rollout.hip"), os.path.join(CSRC, "bmpc_rollout_legs.hip"),
           os.path.join(CSRC, "bmpc_team_rollout_legs.hip"), os.path.join(CSRC, "bmpc_rollout_tune.hip"), os.path.join(CSRC, "bmpc_team_rollout_tune.hip"),
           os.path.join(CSRC, "bmpc_stream_plant.inl"), os.path.join(CSRC, "bmpc_rollout_plant.hip"), os.path.join(CSRC, "bmpc_team_rollout_plant.hip"),
           os.path.join(CSRC, "bmpc_rollout_body.inl"), os.path.join(CSRC, "bmpc_stream_sensor.inl"), os.path.join(CSRC, "bmpc_rollout_sensor.hip"),
           os.path.join(CSRC, "bmpc_team_rollout_sensor.hip"), os.path.join(CSRC, "bmpc_stream_observer.inl"), os.path.join(CSRC, "bmpc_rollout_observer.hip"),
           os.path.join(CSRC, "bmpc_team_rollout_observer.hip")]
# translation units of the library: the one-wave batch kernels + C ABI, the team kernels (NW cooperating waves per problem), the restoration
# kernels (the solver with the restoration phase, continuing what a batch kernel left jammed), the fused closed-loop tick kernels, the pair kernel
# the rollout kernels (many ticks of every stream in one launch), the rollout kernels with events (disturbances, scheduled re-plans) and those with
# events and the audit (tube and joint-limit excess of the state every tick starts from) and those with the logging records on top (path-frame error
# records behind every tick's post, a tracking record per stream), the rollout kernels of the teams (plain and with everything on), the rollout
# kernels with a queue of re-plan records per stream (fired by tick, goal or lost plan) on one wave and on teams, those with a table of controller
# settings per stream on top (sweeps: a grid over settings as one launch) on one wave and on teams, those with a table of actuator models per stream
# between the command and the plant on top of that on one wave and on teams, those with a table of measurement models per stream between the plant and
# the controller on top of that on one wave and on teams, those with a table of state observers per stream between the sensor's sample and the pack on top
# of that on one wave and on teams: 20 units side by side
UNITS = [os.path.join(CSRC, "bmpc_hip.hip"), os.path.join(CSRC, "bmpc_team.hip"), os.path.join(CSRC, "bmpc_resto.hip"), os.path.join(CSRC, "bmpc_tick.hip"),
         os.path.join(CSRC, "bmpc_pair.hip"), os.path.join(CSRC, "bmpc_rollout.hip"), os.path.join(CSRC, "bmpc_rollout_events.hip"),
         os.path.join(CSRC, "bmpc_rollout_audit.hip"), os.path.join(CSRC, "bmpc_rollout_log.hip"), os.path.join(CSRC, "bmpc_team_rollout.hip"),
         os.path.join(CSRC, "bmpc_rollout_legs.hip"), os.path.join(CSRC, "bmpc_team_rollout_legs.hip"), os.path.join(CSRC, "bmpc_rollout_tune.hip"),
         os.path.join(CSRC, "bmpc_team_rollout_tune.hip"), os.path.join(CSRC, "bmpc_rollout_plant.hip"), os.path.join(CSRC, "bmpc_team_rollout_plant.hip"),
         os.path.join(CSRC, "bmpc_rollout_sensor.hip"), os.path.join(CSRC, "bmpc_team_rollout_sensor.hip"), os.path.join(CSRC, "bmpc_rollout_observer.hip"),
         os.path.join(CSRC, "bmpc_team_rollout_observer.hip")]


def hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-mllvm", "-amdgpu-sched-strategy=iterative-ilp",
         "-Wno-unused-variable", "-Wno-unused-value", "-Wno-duplicate-decl-specifier"]
# per-unit flags (none at present; the 256-register experiment of bmpc_pair.hip wanted the default scheduler: 744 B of scratch against 1996 B)
UNIT_FLAGS = {}


def unit_flags(src):
    return UNIT_FLAGS.get(os.path.basename(src), FLAGS)


_COPY = re.compile(r"(v_accvgpr_(write|read)_b32|scratch_(store|load)_\w+|v_mov_b(32|64)(_e32|_e64)?) ")
_HARMLESS = re.compile(r"(s_\w+|v_readlane_b32|v_writelane_b32)( |$)")


def source_hash():
    """Hash of everything the library is built from: the text of every file in SOURCES and the compiler flags.  It is compiled into the
    library (bmpc_build_hash(), and as the marker BMPC_BUILD_HASH=... in its bytes): build() rebuilds when the in-tree library carries another
    hash (not by file times), _lib.load() refuses a library whose hash is not the tree's, and bench.py ties the counter / flop files in
    profiles/ to it."""
    h = hashlib.sha256()
    for p in sorted(SOURCES, key=os.path.basename):
        h.update(os.path.basename(p).encode()); h.update(b"\0")
        with open(p, "rb") as fh:
            h.update(fh.read())
        h.update(b"\0")
    h.update(" ".join(FLAGS).encode())
    for k in sorted(UNIT_FLAGS):
        h.update(("|" + k + ":" + " ".join(UNIT_FLAGS[k])).encode())
    return h.hexdigest()[:16]


def library_hash(path=None):
    """The hash a built library carries (None: no library, or one from before round 5)."""
    path = path or LIB
    if not os.path.exists(path):
        return None
    with open(path, "rb") as fh:
        m = re.search(rb"BMPC_BUILD_HASH=([0-9a-f]{16})", fh.read())
    return m.group(1).decode() if m else None


Ins = collections.namedtuple("Ins", "line text note")                      # text: comment dropped, whitespace collapsed; note: the comment
Block = collections.namedtuple("Block", "label line insns")                # label: "entry", ".LBB0_7" or "bb.7" (a fall-through block)
Function = collections.namedtuple("Function", "name line blocks resources")


def read_listing(asm_path):
    """The functions of a device listing, each with its basic blocks and its resource record: the integer fields of its `amdhsa.kernels`
    metadata entry (vgpr_count, sgpr_spill_count, private_segment_fixed_size, ...) and of its `; Kernel info:` trailer (NumVgprs, NumAgprs,
    Occupancy, ...); empty for a function that is no kernel.  A function runs from its `_Z...:` label to `.Lfunc_end`; `.LBB...:` labels and
    `; %bb.N:` comments open blocks (the listing a full compile saves names the IR block behind them: `.LBB0_7:  ; %Flow5015`); other
    labels, directives and comment lines are no instructions."""
    with open(asm_path) as f:
        listing = f.read()
    funcs, inside = [], False
    for n, s in enumerate(listing.split("\n"), 1):
        s = s.strip()
        m = re.match(r"(_Z\w+):|(\.LBB\w+):|; %bb\.(\d+):", s)
        if m and m.group(1):
            funcs.append(Function(m.group(1), n, [Block("entry", n, [])], {}))
            inside = True
        elif s.startswith(".Lfunc_end"):
            inside = False
        elif not inside:
            m = re.match(r"; (\w+): (\d+)", s)
            if m and funcs:
                funcs[-1].resources[m.group(1)] = int(m.group(2))
        elif m:
            funcs[-1].blocks.append(Block(m.group(2) or "bb." + m.group(3), n, []))
        else:
            text, _, note = s.partition(";")
            text = " ".join(text.split())
            if text and text[0] != "." and text[-1] != ":":
                funcs[-1].blocks[-1].insns.append(Ins(n, text, note.strip()))
    by_name = {fn.name: fn for fn in funcs}
    kernels = set()
    # the metadata (YAML): one `  - .key: value` entry per kernel, its own keys at indent 4, those of its arguments deeper
    for entry in re.split(r"\n  - (?=\.)", listing.partition("\namdhsa.kernels:")[2].partition("\namdhsa.target:")[0])[1:]:
        fields = dict(re.findall(r"^(?:    )?\.(\w+): +(\S+)$", entry, re.M))
        if fields.get("name") in by_name:
            by_name[fields["name"]].resources.update((k, int(v)) for k, v in fields.items() if v.isdigit())
            kernels.add(fields["name"])
    # (a function the kernels CALL -- stream_observe of the observer units -- has a `; Function info:` trailer and no metadata entry: no kernel, no record)
    for fn in funcs:
        if fn.name not in kernels:
            fn.resources.clear()
    return funcs


def lint_isa(asm_path):
    """Static check of the compiled ISA for one register-allocator defect of this toolchain (ROCm 7.2 LLVM) that silently
    corrupts results: a live-range split / spill copy placed at the top of a control-flow join block BEFORE the instruction
    that restores the exec mask (`s_or_b64 exec, exec, s[..]`), so the copy runs only for the lanes of the branch that just
    ended while every lane reads the copy later.  Seen once in this kernel (a prefetched stage input saved to an AGPR under
    the mask of lanes 21..31; DESIGN.md 4, lesson 10): N=30 solves converged to other local minima, nothing crashed.
    Signature: a basic block whose instructions ahead of its first exec restore are only scalar ops and register copies, with
    at least one vector copy among them.  Returns the list of offending (function, block, line, copies)."""
    hits = []
    for fn in read_listing(asm_path):
        for b in fn.blocks:
            texts = [i.text for i in b.insns]
            for j, s in enumerate(texts):
                if s.startswith("s_or_b64 exec, exec, s["):
                    copies = [t for t in texts[:j] if _COPY.match(t)]
                    if copies and all(_COPY.match(t) or _HARMLESS.match(t) for t in texts[:j]):
                        hits.append((fn.name, b.label, b.line, copies))
                    break
    return hits


_LOAD = re.compile(r"^(global_load|ds_read|scratch_load|flat_load|buffer_load)\w*\s+(v\[\d+:\d+\]|v\d+)")
_VREG = re.compile(r"v\[(\d+):(\d+)\]|(?<![a-z_\d])v(\d+)(?!\d)")
_REGION_END = ("s_and_saveexec", "s_andn2_saveexec", "s_or_saveexec", "s_xor_b64 exec", "s_endpgm", "s_branch", "s_setpc")
_STORES = ("global_store", "ds_write", "scratch_store", "flat_store", "buffer_store", "global_atomic", "ds_add")


def _vregs(text):
    out = set()
    for m in _VREG.finditer(text):
        out |= set(range(int(m.group(1)), int(m.group(2)) + 1)) if m.group(1) else {int(m.group(3))}
    return out


def _defs_uses(s):
    parts = s.split(None, 1)
    if len(parts) < 2:
        return set(), set()
    mn, ops = parts[0], [o.strip() for o in parts[1].split(",")]
    if mn.startswith(_STORES) or (mn.startswith(("s_", "v_cmp", "v_readlane", "v_readfirstlane")) and not mn.startswith("v_cmpx")):
        return set(), set().union(*[_vregs(o) for o in ops])
    d = _vregs(ops[0])
    u = set().union(*[_vregs(o) for o in ops[1:]]) if len(ops) > 1 else set()
    if mn.startswith(("v_fmac", "v_mac", "v_dot", "v_mfma", "v_writelane")):
        u |= d
    return d, u


def lint_isa_masked_loads(asm_path, window=400):
    """Second signature of the same toolchain's trouble with control flow (`cond ? state[i] : 0.0` on a possibly null
    pointer compiled into an exec-masked load whose join lost the other arm): a register whose only definition near a join is a LOAD
    executed under `s_and_saveexec` and which is READ after the matching `s_or_b64 exec, exec, ...` -- the lanes the mask switched
    off read whatever the register held.  For every such region (single block, no nested control flow) the loaded registers must
    have been written in the straight-line code ahead of the saveexec (the default arm: `v_mov`, `v_cndmask`, ...).
    Returns [(function, line of the saveexec, registers, defined_earlier)]: `defined_earlier` says whether the function writes the
    register anywhere before (in listing order) -- then the register may legitimately hold the default from further back (a long-lived
    value) and the hit is only a candidate; with no earlier write at all the inactive lanes certainly read garbage."""
    hits = []
    for fn in read_listing(asm_path):
        lines = []      # of the function: (line, text, False) per instruction, (line, "", True) where a label opens a block
        for b in fn.blocks:
            if b.label.startswith(".LBB"):
                lines.append((b.line, "", True))
            lines += [(i.line, i.text, False) for i in b.insns]
        n = len(lines)
        seen = set()       # registers written so far in listing order
        written_before = []
        for (_, s, _) in lines:
            written_before.append(set(seen))
            seen |= _defs_uses(s)[0] if s else set()
        for i, (ln, s, _) in enumerate(lines):
            # only `if` regions without an else arm: an else arm (s_andn2_saveexec / s_or_saveexec on the xor-ed mask) complements a then
            # arm that defined the register for the other lanes
            m = re.match(r"s_and_saveexec_b64 (s\[\d+:\d+\])", s)
            if not m:
                continue
            save, loads, j, closed = m.group(1), set(), i + 1, False
            while j < n and j < i + window:
                sj = lines[j][1]
                if sj.startswith("s_or_b64 exec, exec, " + save):
                    closed = True
                    break
                if sj.startswith(_REGION_END):
                    break
                d, _u = _defs_uses(sj)
                lm = _LOAD.match(sj)
                if lm:
                    loads |= _vregs(lm.group(2))
                else:
                    loads -= d          # recomputed inside the region: no longer a bare load result
                j += 1
            if not closed or not loads:
                continue
            pre, k = set(), i - 1
            while k >= 0 and k > i - window:      # straight-line code ahead of the saveexec (up to the previous label / branch / join)
                sk = lines[k][1]
                if lines[k][2] or sk.startswith(("s_or_b64 exec", "s_cbranch", "s_branch")):
                    break
                pre |= _defs_uses(sk)[0]
                k -= 1
            cand = loads - pre
            live, used, k = set(cand), set(), j + 1
            while k < n and k < j + window and live:
                sk = lines[k][1]
                if lines[k][2] or sk.startswith(("s_endpgm", "s_branch", "s_setpc", "s_cbranch")):
                    break
                d, u = _defs_uses(sk)
                used |= u & live
                live -= d
                k += 1
            if used:
                hits.append((fn.name, ln, sorted(used), bool(used & written_before[i]) and used <= written_before[i]))
    return hits


def compile_unit(src, out_dir, defines=(), lint=True, verbose=False):
    """ONE compiler run for a translation unit: leaves in out_dir the object <unit>.o (returned), the device listing of that same compilation
    <unit>_gfx950.s (`-save-temps=obj`: the object's device code is assembled from exactly this text) and the dependency file <unit>.d.
    The lints read that listing; a hit fails the build (the compiled code would compute wrong numbers for some lanes)."""
    stem = os.path.splitext(os.path.basename(src))[0]
    obj, asm, dep = (os.path.join(out_dir, stem + e) for e in (".o", "_gfx950.s", ".d"))
    os.makedirs(out_dir, exist_ok=True)
    # -amdgpu-sched-strategy=iterative-ilp: the solver runs at one wave per SIMD, so the scheduler should chase instruction-level
    # parallelism (loads hoisted ahead of their uses), not occupancy; measured 12.7 -> 10.8 ms at B=1024 (profiles/)
    cmd = [hipcc()] + unit_flags(src) + ["-DBMPC_BUILD_HASH_STR=\"%s\"" % source_hash()] + list(defines) + \
          ["-fPIC", "-save-temps=obj", "-MD", "-MF", dep, "-c", "-o", obj, src]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd, cwd=CSRC)
    os.replace(os.path.join(out_dir, stem + "-hip-amdgcn-amd-amdhsa-gfx950.s"), asm)
    for pat in (stem + "-hip-amdgcn-*", stem + "-host-*", os.path.basename(src) + "-hip-*"):      # the other temporaries (.hipi, .bc, host .s, ...)
        for tmp in glob.glob(os.path.join(out_dir, pat)):
            os.remove(tmp)
    if lint:
        bad = lint_isa(asm)
        if bad:
            raise RuntimeError("ISA lint: register copies ahead of an exec-mask restore (compiler defect, results would be wrong): %r" % (bad,))
        # masked loads read after their join: fatal in EVERY kernel of the library (round 4: the last source pattern that produced a candidate
        # -- `cond ? plan[...] : value` in the stream post-processing -- loads unconditionally behind an opaque barrier now, so the listing of
        # the shipped text has no hit at all and a new one is a change worth stopping for)
        ml = lint_isa_masked_loads(asm)
        if ml:
            raise RuntimeError("ISA lint: load under an exec mask whose result is read after the join (results may be wrong for the masked-off "
                               "lanes; `defined_earlier` = the register has an earlier definition in listing order): %r" % (ml,))
    return obj


def sources_mismatch(deps, sources=None):
    """SOURCES against what the compiler read: (missing, superfluous) = the files of this tree among `deps` (paths as in the dependency
    files, relative ones taken from csrc/) that SOURCES lacks -- a change to one would not change source_hash(), and a stale library would
    load -- and the files of SOURCES that no unit read."""
    root = os.path.realpath(os.path.join(HERE, ".."))
    read = {os.path.realpath(os.path.join(CSRC, d)) for d in deps}
    read = {d for d in read if d.startswith(root + os.sep)}
    listed = {os.path.realpath(p) for p in (SOURCES if sources is None else sources)}
    return sorted(os.path.relpath(d, root) for d in read - listed), sorted(os.path.relpath(d, root) for d in listed - read)


def build(force=False, verbose=False, lint=True, lib=LIB, out_dir=ISA_DIR, defines=()):
    """The units side by side, one compile_unit() each, the SOURCES check on their dependency files, and the link (lib, out_dir, defines: the
    diagnostic builds of tests/)."""
    if not force and library_hash(lib) == source_hash():      # the library in the tree was built from exactly this text with these flags
        return lib
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(len(UNITS)) as ex:
        objs = list(ex.map(lambda src: compile_unit(src, out_dir, defines, lint, verbose), UNITS))
    deps = []
    for obj in objs:
        with open(obj[:-2] + ".d") as f:      # make syntax: `<object>: file file \` and so on, blanks in names escaped
            deps += shlex.split(f.read().replace("\\\n", " "))[1:]
    missing, superfluous = sources_mismatch(deps)
    if missing or superfluous:
        raise RuntimeError("build.SOURCES is not what the units read: missing %r, superfluous %r" % (missing, superfluous))
    subprocess.check_call([hipcc(), "--offload-arch=gfx950", "-fPIC", "-shared", "-o", lib] + objs, cwd=CSRC)
    return lib


def digest(asm_dir=ISA_DIR):
    """[(listing, kernel, instructions, digest)] for every function with instructions in the listings of asm_dir: the first 16 hex digits
    of the SHA-256 of its block labels and instruction texts as read_listing() normalises them (no comments, directives or `__hip_cuid_*`
    label, whitespace collapsed).  Equal digests are what "the device listings equal the parent's" means."""
    rows = []
    for asm in sorted(glob.glob(os.path.join(asm_dir, "*_gfx950.s"))):
        for fn in read_listing(asm):
            stream = [t for b in fn.blocks for t in [b.label + ":"] * b.label.startswith(".LBB") + [i.text for i in b.insns]]
            count = sum(len(b.insns) for b in fn.blocks)
            if count:
                rows.append((os.path.basename(asm), fn.name, count, hashlib.sha256("\n".join(stream).encode()).hexdigest()[:16]))
    return rows


if __name__ == "__main__":
    if "--digest" in sys.argv:
        for row in digest(*sys.argv[sys.argv.index("--digest") + 1:][:1]):
            print("%s %s %d %s" % row)
    else:
        build(force="--force" in sys.argv, verbose=True)
        print(LIB)
