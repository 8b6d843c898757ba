"""Diagnostic (CPU, needs hipcc only when it has to build): the resource table of every kernel of libboundmpc_hip.so, from the listings the build
left in build/isa (boundmpc_amd.build.read_listing: the kernels' metadata and `; Kernel info:` trailers) -- registers, AGPRs, scratch per lane,
SGPR / VGPR spills, LDS, occupancy.  DESIGN.md 4 quotes THIS output (profiles/rNN_kernel_resources.txt) instead of numbers copied by hand.
Usage: python tests/kernel_resources.py      (builds first when the library is stale or the listings are missing)"""
import os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from boundmpc_amd import build      # noqa: E402

listings = [os.path.join(build.ISA_DIR, os.path.splitext(os.path.basename(u))[0] + "_gfx950.s") for u in build.UNITS]
build.build(force=not all(os.path.exists(a) for a in listings))
rows = [fn for a in listings for fn in build.read_listing(a) if fn.resources]
names = {"_Z17bmpc_solve_kernelILb1EE": "bmpc_solve_kernel<ZLDS=true> (batch, N<=11, S<=4: the headline's)", "_Z17bmpc_solve_kernelILb0EE": "bmpc_solve_kernel<false> (batch, long horizons / S>4)",
         "_Z17bmpc_resto_kernelILb1EE": "bmpc_resto_kernel<true> (restoration, continues jammed problems)", "_Z17bmpc_resto_kernelILb0EE": "bmpc_resto_kernel<false>",
         "_Z22bmpc_team_solve_kernel": "bmpc_team_solve_kernel (batch, 4 waves per problem)", "_Z21bmpc_team_tick_kernelILb1EE": "bmpc_team_tick_kernel<RESTO=true> (fused tick, teams)",
         "_Z21bmpc_team_tick_kernelILb0EE": "bmpc_team_tick_kernel<false> (time-budgeted ticks)", "_Z23bmpc_stream_tick_kernelILb1ELb1EE": "bmpc_stream_tick_kernel<ZLDS=true, RESTO=true>",
         "_Z23bmpc_stream_tick_kernelILb1ELb0EE": "bmpc_stream_tick_kernel<true, false>", "_Z23bmpc_stream_tick_kernelILb0ELb1EE": "bmpc_stream_tick_kernel<false, true>",
         "_Z23bmpc_stream_tick_kernelILb0ELb0EE": "bmpc_stream_tick_kernel<false, false>", "_Z22bmpc_pair_solve_kernel": "bmpc_pair_solve_kernel (batch, 2 waves per problem, 256 < B <= 512)", "_Z18queue_order_kernel": "queue_order_kernel (ranking of a long-horizon batch)",
         "_Z19bmpc_service_kernelILb1EN4bmpc9DualBatchE": "bmpc_service_kernel<ZLDS=true, DualBatch> (dual state from multipliers)", "_Z19bmpc_service_kernelILb0EN4bmpc9DualBatchE": "bmpc_service_kernel<false, DualBatch>",
         "_Z19bmpc_service_kernelILb1EN4bmpc8KktBatchE": "bmpc_service_kernel<true, KktBatch> (KKT certificate)", "_Z19bmpc_service_kernelILb0EN4bmpc8KktBatchE": "bmpc_service_kernel<false, KktBatch>",
         "_Z19bmpc_service_kernelILb1EN4bmpc9SensBatchE": "bmpc_service_kernel<true, SensBatch> (parametric sensitivity)", "_Z19bmpc_service_kernelILb0EN4bmpc9SensBatchE": "bmpc_service_kernel<false, SensBatch>",
         "_Z23bmpc_stream_pack_kernel": "bmpc_stream_pack_kernel", "_Z23bmpc_stream_post_kernel": "bmpc_stream_post_kernel"}
print(f"kernel resources of libboundmpc_hip.so, source hash {build.source_hash()} (listings of the build in build/isa; flags: {' '.join(build.FLAGS)})")
print("%-78s %5s %5s %8s %6s %6s %8s %4s" % ("kernel", "VGPR", "AGPR", "scratch", "sgprS", "vgprS", "LDS B", "occ"))
seen = set()
for r in rows:
    label = next((v for k, v in names.items() if r.name.startswith(k)), r.name[:70])
    if label in seen:
        continue
    seen.add(label)
    res = r.resources
    print("%-78s %5d %5d %6d B %6d %6d %8d %4d" % (label, res["NumVgprs"], res["NumAgprs"], res["private_segment_fixed_size"], res["sgpr_spill_count"], res["vgpr_spill_count"],
                                                   res["group_segment_fixed_size"], res["Occupancy"]))
