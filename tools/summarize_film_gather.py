"""tools/profile_film_gather.sh's summary: the counters of the film gather launches of one render pass, summed over the launches,
and per camera sample (width x height x spp of the workload)."""
import csv, json, os, sys

out_dir, tag = sys.argv[1], sys.argv[2]
sys.path.insert(0, ".")
from nori_amd import workloads
sc = workloads.load(os.environ.get("WORKLOAD", "pa4-cbox-path_mis")).scene
samples = sc.camera.width * sc.camera.height * sc.sample_count
res = {"tag": tag, "gather_switch": os.environ.get("NORI_HIP_FILM_GATHER", ""), "samples": samples, "kernel": None, "launches": 0, "counters": {}}
for name in ("lds", "elapsed"):
    path = os.path.join(out_dir, name + "_counter_collection.csv")
    if not os.path.exists(path):
        continue
    seen = set()
    for row in csv.DictReader(open(path)):
        if "film_gather" not in row["Kernel_Name"]:
            continue
        res["kernel"] = row["Kernel_Name"][:120]
        res["workgroup_size"], res["lds_block_size"], res["vgpr_count"] = int(row["Workgroup_Size"]), int(row["LDS_Block_Size"]), int(row["VGPR_Count"])
        res["counters"][row["Counter_Name"]] = res["counters"].get(row["Counter_Name"], 0.0) + float(row["Counter_Value"])
        if name == "lds":
            seen.add(row["Dispatch_Id"])
    if name == "lds":
        res["launches"] = len(seen)
res["per_sample"] = {k: v / samples for k, v in res["counters"].items() if k.startswith("SQ_INSTS") or k.startswith("SQ_LDS")}
print(json.dumps(res, indent=1))
