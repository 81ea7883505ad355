#!/usr/bin/env python3
"""Vector-ALU against MFMA occupancy of the conv kernels, from one rocprofv3 counter pass (counters alone, no tracing flags):

    rocprofv3 --pmc SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_VALU_MFMA_BUSY_CYCLES SQ_VALU_MFMA_COEXEC_CYCLES SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_WAIT_ANY \\
        SQ_WAIT_INST_ANY -d DIR -o run --output-format csv -- python3 bench.py --gpus 1 --steps 20 --warmup 5 --no-graph
    python tools/pmc_valu.py DIR [name-substring ...]        (default: the conv kernels)

Per kernel, averaged over its launches: the raw counters, and as shares of the SIMD cycles (1024 SIMDs x SQ_BUSY_CYCLES / 32 shader engines, as in
tools/pmc_sq.py) the MFMA pipe's busy cycles and the cycles the arbiter spent on vector-ALU instructions (SQ_ACTIVE_INST_VALU counts quad-cycles: x 4)."""
import collections, csv, glob, os, sys
f = max(glob.glob(os.path.join(sys.argv[1], "**", "*counter_collection.csv"), recursive=True), key=os.path.getmtime)
want = sys.argv[2:] or ["conv_wgrad_kernel", "wgrad_c1_kernel", "down_c1_vec", "conv_data_kernel"]
per = collections.OrderedDict()
for r in csv.DictReader(open(f)):
    e = per.setdefault(int(r["Dispatch_Id"]), [r["Kernel_Name"], {}])
    e[1][r["Counter_Name"]] = e[1].get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
agg = {}
for n, c in per.values():
    if any(k in n for k in want):
        a = agg.setdefault(n[:70], collections.Counter()); a.update(c); a["_n"] += 1
for k, a in sorted(agg.items(), key=lambda kv: -kv[1]["SQ_BUSY_CYCLES"]):
    n, cyc = a["_n"], a["SQ_BUSY_CYCLES"] / 32.0
    simd_cyc = 1024 * cyc
    print(k, "launches", int(n))
    for c in sorted(a):
        if c != "_n":
            print(f"   {c:32s} {a[c] / n:16.0f} per launch")
    print(f"   kernel cycles (SQ_BUSY / 32)     {cyc / n:16.0f}")
    print(f"   MFMA busy / SIMD cycles          {100 * a['SQ_VALU_MFMA_BUSY_CYCLES'] / simd_cyc:8.1f} %")
    print(f"   4 ACTIVE_INST_VALU / SIMD cycles {100 * 4 * a['SQ_ACTIVE_INST_VALU'] / simd_cyc:8.1f} %")
    print(f"   COEXEC / MFMA busy               {100 * a['SQ_VALU_MFMA_COEXEC_CYCLES'] / max(a['SQ_VALU_MFMA_BUSY_CYCLES'], 1):8.1f} %")
    print(f"   WAIT_ANY / WAVE_CYCLES           {100 * a['SQ_WAIT_ANY'] / max(a['SQ_WAVE_CYCLES'], 1):8.1f} %")
    print(f"   WAIT_INST_ANY / WAVE_CYCLES      {100 * a['SQ_WAIT_INST_ANY'] / max(a['SQ_WAVE_CYCLES'], 1):8.1f} %")
