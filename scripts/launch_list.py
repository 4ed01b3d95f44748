"""A kernel trace (the CSVs `rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/tower_ab.py --child OUT.npz` leaves under
DIR) as the ordered list of (kernel, grid, workgroup) in dispatch order, one launch per line, and its summary: the number of launches, the
SHA-256 of the ordered list and the launches per kernel.  Two libraries that make the same launches in the same order give the same
digest; the summary is what profiles/host_seq/ keeps (the list itself is some 10,000 lines).  The HIP runtime's own copy / fill kernels
(__amd_rocclr_*) are left out: they serve the callers' hipMemcpy / hipMemset, and how the runtime splits a copy varies from run to run.
usage: launch_list.py TRACE_DIR LIST.txt SUMMARY.txt"""
import collections, csv, glob, hashlib, sys
rows = []
for f in glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True):
    with open(f, newline="") as fh:
        for r in csv.DictReader(fh):
            name = r["Kernel_Name"].split("(")[0].strip()
            if not name.startswith("__amd_rocclr_"):
                rows.append((int(r["Dispatch_Id"]), name, "x".join(r[f"Grid_Size_{a}"] for a in "XYZ"), "x".join(r[f"Workgroup_Size_{a}"] for a in "XYZ")))
rows.sort()
lines = [f"{name} {grid} {wg}\n" for _, name, grid, wg in rows]
with open(sys.argv[2], "w") as out:
    out.writelines(lines)
per_kernel = collections.Counter(name for _, name, _, _ in rows)
with open(sys.argv[3], "w") as out:
    out.write(f"{len(lines)} kernel launches in dispatch order, {len(set(lines))} distinct (kernel, grid, workgroup)\n")
    out.write(f"sha256 of the ordered list, one `kernel grid workgroup` line per launch: {hashlib.sha256(''.join(lines).encode()).hexdigest()}\n")
    for name, n in sorted(per_kernel.items()): out.write(f"{n:6d}  {name}\n")
print(open(sys.argv[3]).read().split("\n", 2)[0])
