"""Residency of the encode launches in one rocprofv3 counter pass
(tools/gpu_run.sh pmc: over tools/prof_bench.py): launch time, clock,
resident waves per CU (wave-cycles per CU-cycle; SQ wave counters count
quad-cycles, GRBM_GUI_ACTIVE sums the 8 XCDs), wave-cycles per block and the
share of them spent waiting on data.

    python tools/enc_occ_summary.py profiles/enc_occ/pmc_new/run_counter_collection.csv
"""
import csv
import sys
from collections import defaultdict

CUS, XCDS = 256, 8


def main():
    launches = defaultdict(dict)
    for r in csv.DictReader(open(sys.argv[1])):
        if "encode_blocks_kernel" not in r["Kernel_Name"]:
            continue
        v = launches[int(r["Dispatch_Id"])]
        v[r["Counter_Name"]] = float(r["Counter_Value"])
        v["ns"] = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        v["lds"] = int(r["LDS_Block_Size"])
        v["blocks"] = int(r["Grid_Size"]) // max(int(r["Workgroup_Size"]), 1)
    for d, v in sorted(launches.items()):
        cycles = v["GRBM_GUI_ACTIVE"] / XCDS  # of the launch, per XCD
        wave_cycles = 4.0 * v["SQ_WAVE_CYCLES"]
        print(f"dispatch {d}: {v['blocks']} blocks, LDS {v['lds']} B (as the profiler rounds it), "
              f"{v['ns'] / 1e6:.3f} ms at {cycles / v['ns']:.2f} GHz = {cycles / 1e6:.2f} M cycles; "
              f"resident waves per CU {wave_cycles / (cycles * CUS):.2f}; "
              f"wave-cycles per block {wave_cycles / v['blocks'] / 1e3:.0f} K; "
              f"waiting on data {v.get('SQ_WAIT_ANY', 0) / v['SQ_WAVE_CYCLES']:.2f}")


if __name__ == "__main__":
    main()
