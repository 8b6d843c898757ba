"""The C-ABI shared library loads and exports every symbol include/boundmpc_hip.h declares (no compute calls).
Also: without a GPU the product refuses to construct a solver -- there is no CPU fallback."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    txt = open(os.path.join(ROOT, "include", "boundmpc_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(bmpc_[a-z_]+)\s*\(", txt)))


def test_header_symbols_exported():
    from boundmpc_amd import _lib, build
    build.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared()
    assert len(names) >= 12
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/boundmpc_hip.h but not exported"
    assert sorted(_lib.SYMBOLS) == names


def test_options_and_error_strings():
    from boundmpc_amd import _lib
    lib = _lib.load()
    o = _lib.Options()
    assert lib.bmpc_default_options(ctypes.byref(o)) == 0
    assert o.tol == 1e-8 and o.max_iter == 500 and o.exact_hessian == 1
    assert lib.bmpc_error_string(0) == b"ok" and lib.bmpc_error_string(4) == b"no HIP device available"
    h = ctypes.c_void_p()
    assert lib.bmpc_create(0, 4, 0.1, None, ctypes.byref(h)) == 1      # invalid N
    assert lib.bmpc_create(10, 9, 0.1, None, ctypes.byref(h)) == 1     # invalid S


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from boundmpc_amd import BatchedOCPSolver, BoundMPCHipError
    with pytest.raises(BoundMPCHipError):
        BatchedOCPSolver(10, 4, 0.1)


def test_product_does_not_reference_oracle_or_emulator():
    """The product package must never import, link or execute anything under oracle/ or tests/."""
    pkg = os.path.join(ROOT, "boundmpc_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".hip", ".inl", ".h", ".cpp")):
                src = open(os.path.join(dp, f)).read()
                for pat in (r"^\s*(from|import)\s+oracle", r"^\s*(from|import)\s+tests", r"libbmpc_oracle", r"libbmpc_emu"):
                    assert not re.search(pat, src, flags=re.M), f"{f} refers to test infrastructure ({pat})"


def _unit_listings(b):
    """the device listings of the library's five units, where a build has left them (a library that came with the tree has none)"""
    paths = [os.path.join(b.ISA_DIR, os.path.splitext(os.path.basename(u))[0] + "_gfx950.s") for u in b.UNITS]
    return [p for p in paths if os.path.exists(p)]


def test_isa_lint_flags_copies_ahead_of_exec_restore(tmp_path):
    """build.lint_isa: the signature of the register-allocator defect described in DESIGN.md 4 (copies ahead of the exec
    restore of a join block) is flagged, ordinary join blocks are not; the ISA of the shipped library is clean."""
    from boundmpc_amd import build as b
    bad = """_Z6kernelv:
; %bb.0:
	s_and_saveexec_b64 s[12:13], s[0:1]
; %bb.1:
	v_add_f64 v[0:1], v[2:3], v[4:5]
; %bb.2:                                ; %Flow4706
                                        ;   in Loop: Header=BB0_3 Depth=1
	s_waitcnt vmcnt(4)
	v_accvgpr_write_b32 a149, v9
	v_accvgpr_write_b32 a148, v8
	s_mov_b32 s25, s63
	s_or_b64 exec, exec, s[12:13]
	v_mov_b64_e32 v[26:27], 0
.LBB0_3:                                ; %Flow5016
	v_readlane_b32 s4, v255, 34
	s_or_b64 exec, exec, s[4:5]
	v_accvgpr_write_b32 a1, v2
.LBB0_4:
	v_cmp_lt_f64_e64 vcc, v[0:1], v[2:3]
	v_accvgpr_read_b32 v52, a92
	s_or_b64 exec, exec, s[6:7]
	s_endpgm
"""
    f = tmp_path / "k.s"
    f.write_text(bad)
    hits = b.lint_isa(str(f))
    assert len(hits) == 1 and hits[0][1] == "bb.2" and len(hits[0][3]) == 2
    for asm in _unit_listings(b):
        assert b.lint_isa(asm) == []


def test_isa_lint_flags_masked_load_read_after_its_join(tmp_path):
    """build.lint_isa_masked_loads: the second miscompile signature of DESIGN.md 4 (`cond ? p[i] : 0.0` lowered to a load under an exec
    mask whose join lost the other arm): a register defined only by a masked load and read after the exec restore is flagged; the
    correct lowering (default written ahead of the saveexec) and a load consumed inside its region are not."""
    from boundmpc_amd import build as b
    bad = """_Z6kernelv:
; %bb.0:
	v_cmp_gt_i32_e32 vcc, 7, v0
	s_and_saveexec_b64 s[2:3], vcc
	s_cbranch_execz .LBB0_2
; %bb.1:
	global_load_dwordx2 v[4:5], v[2:3], off offset:232
.LBB0_2:                                ; %Flow
	s_or_b64 exec, exec, s[2:3]
	s_waitcnt vmcnt(0)
	v_fma_f64 v[6:7], v[4:5], v[8:9], v[10:11]
	s_endpgm
_Z5good1v:
; %bb.0:
	v_mov_b64_e32 v[4:5], 0
	v_cmp_gt_i32_e32 vcc, 7, v0
	s_and_saveexec_b64 s[2:3], vcc
	s_cbranch_execz .LBB1_2
; %bb.1:
	global_load_dwordx2 v[4:5], v[2:3], off offset:232
.LBB1_2:
                                        ; %Flow12
	s_or_b64 exec, exec, s[2:3]
	s_waitcnt vmcnt(0)
	v_fma_f64 v[6:7], v[4:5], v[8:9], v[10:11]
	s_endpgm
_Z5good2v:
; %bb.0:
	s_and_saveexec_b64 s[2:3], vcc
	s_cbranch_execz .LBB2_2
; %bb.1:
	ds_read_b64 v[4:5], v1 offset:64
	s_waitcnt lgkmcnt(0)
	global_store_dwordx2 v[2:3], v[4:5], off
.LBB2_2:
	s_or_b64 exec, exec, s[2:3]
	v_mov_b64_e32 v[4:5], 0
	v_add_f64 v[6:7], v[4:5], v[8:9]
	s_endpgm
"""
    f = tmp_path / "m.s"
    f.write_text(bad)
    hits = b.lint_isa_masked_loads(str(f))
    assert len(hits) == 1 and hits[0][0] == "_Z6kernelv" and hits[0][2] == [4, 5] and hits[0][3] is False
    for asm in _unit_listings(b):      # the shipped kernels have no such region at all (round 4)
        assert b.lint_isa_masked_loads(asm) == []


_LISTING = """	.text
	.globl	_Z6kernelv
	.type	_Z6kernelv,@function
_Z6kernelv:                             ; @_Z6kernelv
; %bb.0:
	s_load_dwordx2 s[0:1], s[4:5], 0x0
	v_cmp_gt_i32_e32 vcc, 7, v0
	s_and_saveexec_b64 s[2:3], vcc
	s_cbranch_execz .LBB0_2
; %bb.1:COMMENT_A
	global_load_dwordx2	 v[4:5], v[2:3], off offset:232 ; 8-byte Folded Reload
.LBB0_2:COMMENT_B
	s_or_b64 exec, exec, s[2:3]
	s_endpgm
	.section	.rodata,"a",@progbits
	.amdhsa_kernel _Z6kernelv
		.amdhsa_next_free_vgpr 12
	.end_amdhsa_kernel
	.text
.Lfunc_end0:
	.size	_Z6kernelv, .Lfunc_end0-_Z6kernelv
                                        ; -- End function
	.set _Z6kernelv.num_vgpr, 12
; Kernel info:
; codeLenInByte = 48
; NumVgprs: 12
; NumAgprs: 4
; ScratchSize: 444
; LDSByteSize: 40896 bytes/workgroup (compile time only)
; Occupancy: 1
	.type	__hip_cuid_CUID,@object
__hip_cuid_CUID:
	.byte	0
	.amdgpu_metadata
---
amdhsa.kernels:
  - .agpr_count:     4
    .args:
      - .offset:         0
        .size:           280
        .value_kind:     by_value
    .group_segment_fixed_size: 40896
    .name:           _Z6kernelv
    .private_segment_fixed_size: 444
    .sgpr_spill_count: 454
    .symbol:         _Z6kernelv.kd
    .vgpr_count:     16
    .vgpr_spill_count: 148
amdhsa.target:   amdgcn-amd-amdhsa--gfx950
amdhsa.version:
  - 1
  - 2
...

	.end_amdgpu_metadata
"""


def _listing(tmp_path, name, cuid="85b2a929ab681589", a="", b="", text=_LISTING):
    d = tmp_path / name
    d.mkdir()
    (d / "k_gfx950.s").write_text(text.replace("CUID", cuid).replace("COMMENT_A", a).replace("COMMENT_B", b))
    return str(d)


def test_listing_reader_returns_blocks_and_the_resource_record(tmp_path):
    """build.read_listing: blocks with their labels, lines and instruction texts (comments dropped, whitespace collapsed); the resource
    record joins the kernel's metadata entry (not the keys of its arguments) with the `; Kernel info:` trailer."""
    from boundmpc_amd import build as b
    fn, = b.read_listing(os.path.join(_listing(tmp_path, "a", b="                                ; %Flow"), "k_gfx950.s"))
    assert fn.name == "_Z6kernelv" and [(k.label, k.line, len(k.insns)) for k in fn.blocks] == [("entry", 4, 0), ("bb.0", 5, 4), ("bb.1", 10, 1), (".LBB0_2", 12, 2)]
    assert fn.blocks[2].insns[0] == (11, "global_load_dwordx2 v[4:5], v[2:3], off offset:232", "8-byte Folded Reload")
    r = fn.resources
    assert (r["NumVgprs"], r["NumAgprs"], r["Occupancy"], r["ScratchSize"], r["LDSByteSize"]) == (12, 4, 1, 444, 40896)
    assert (r["vgpr_count"], r["agpr_count"], r["private_segment_fixed_size"], r["group_segment_fixed_size"], r["sgpr_spill_count"], r["vgpr_spill_count"]) == (16, 4, 444, 40896, 454, 148)
    assert "offset" not in r and "size" not in r and "name" not in r


def test_digest_ignores_comments_and_the_cuid_label_not_an_instruction(tmp_path):
    """build.digest, the definition of "the device listings equal the parent's": the listing of a plain -S compile and the one a full compile
    saves (`; %Flow` block names, on the header's line or their own; another `__hip_cuid_` label) have equal digests; one changed operand or
    one moved label does not."""
    from boundmpc_amd import build as b
    plain = b.digest(_listing(tmp_path, "plain"))
    saved = b.digest(_listing(tmp_path, "saved", cuid="0123456789abcdef", a="                                ; %Flow4706",
                              b="\n                                        ; %Flow\n                                        ;   in Loop: Header=BB0_3 Depth=1"))
    assert plain == saved and len(plain) == 1 and plain[0][:3] == ("k_gfx950.s", "_Z6kernelv", 7) and len(plain[0][3]) == 16
    operand = b.digest(_listing(tmp_path, "operand", text=_LISTING.replace("offset:232", "offset:240")))
    label = b.digest(_listing(tmp_path, "label", text=_LISTING.replace(".LBB0_2:COMMENT_B\n\ts_or_b64 exec, exec, s[2:3]\n", "\ts_or_b64 exec, exec, s[2:3]\n.LBB0_2:\n")))
    assert operand[0][2] == label[0][2] == 7 and len({plain[0][3], operand[0][3], label[0][3]}) == 3


def test_sources_check_names_a_dropped_and_an_extra_file():
    """build.sources_mismatch: SOURCES against the files the compiler's dependency files name -- a file the units read that SOURCES lacks (its
    changes would not change the hash) and a file of SOURCES nobody reads are both reported by name; files outside the tree do not count."""
    from boundmpc_amd import build as b
    deps = [os.path.relpath(p, b.CSRC) if i % 2 else p for i, p in enumerate(b.SOURCES)] + ["/opt/rocm/include/hip/hip_runtime.h"]
    assert b.sources_mismatch(deps) == ([], [])
    dropped = [p for p in b.SOURCES if not p.endswith("bmpc_kkt.inl")]
    assert b.sources_mismatch(deps, dropped) == ([os.path.join("boundmpc_amd", "csrc", "bmpc_kkt.inl")], [])
    extra = b.SOURCES + [os.path.join(b.CSRC, "bmpc_gone.inl")]
    assert b.sources_mismatch(deps, extra) == ([], [os.path.join("boundmpc_amd", "csrc", "bmpc_gone.inl")])
    assert b.sources_mismatch(deps[1:]) == ([], [os.path.join("boundmpc_amd", "csrc", "bmpc_hip.hip")])


def test_library_carries_the_hash_of_its_sources(tmp_path, monkeypatch):
    """Round 5: the library is tied to the text it was built from.  build.source_hash() covers every source file and the compiler flags; the built
    library carries it (bmpc_build_hash, and as a marker in its bytes, which build() reads instead of file times); _lib.load() refuses an in-tree
    library whose hash differs; bench.kernel_text_hash -- the key of profiles/pmc_current.json and flops_current.json -- is the same hash."""
    import bench
    from boundmpc_amd import _lib, build
    build.build()
    want = build.source_hash()
    assert re.fullmatch(r"[0-9a-f]{16}", want) and build.library_hash() == want and bench.kernel_text_hash() == want
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.bmpc_build_hash.restype = ctypes.c_char_p
    assert lib.bmpc_build_hash().decode() == want and lib.bmpc_options_size() == ctypes.sizeof(_lib.Options)
    # every translation unit and every header the kernels include is part of the hash
    names = {os.path.basename(p) for p in build.SOURCES}
    assert {"bmpc_hip.hip", "bmpc_team.hip", "bmpc_resto.hip", "bmpc_tick.hip", "bmpc_wave.inl", "bmpc_stream.inl", "bmpc_gpu_common.h", "boundmpc_hip.h",
            "bmpc_pair.hip", "bmpc_multi_batch.inl", "bmpc_tick_kernel.inl", "bmpc_args.h"} <= names
    # a library from other sources is refused at load time
    monkeypatch.setattr(build, "source_hash", lambda: "0" * 16)
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(_lib.BoundMPCHipError, match="built from other sources"):
        _lib.load()
    monkeypatch.undo()
    _lib._lib = None
    assert _lib.load() is not None
