#!/usr/bin/env python3
"""DESIGN.md = docs/_parts/*.md with the @TOKENS@ of the state table and of section 5 filled from the profile round's files under profiles/
(tools/profile_round.sh r06): so the numbers in the document are the ones in the committed JSON files, not retyped ones."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
P = os.path.join(ROOT, "profiles")
TAG = sys.argv[1] if len(sys.argv) > 1 else "r06"


def last(name):
    with open(os.path.join(P, name)) as f:
        return json.loads(f.read().strip().splitlines()[-1])


b, h, s128, s16 = last(f"{TAG}_bench.json"), last(f"{TAG}_bench_hdl64.json"), last(f"{TAG}_bench_s128.json"), last(f"{TAG}_bench_s16.json")
st = {k: last(f"{TAG}_stream_input{k}.json") for k in ("", "_s128", "_16_byte_points", "_s128_16_byte_points")}
lat = last(f"{TAG}_latency.json")
pt = json.load(open(os.path.join(P, "pmc_traffic.json")))
r = b["roofline"]; km = r["kernel_ms_per_step"]; gb = r["kernel_algorithmic_GBps"]; iss = r["issue"]
batch = b["config"]["scans_per_gpu_per_step"]
ORDER = ["k_organize", "k_ring_pick", "k_ring_features", "k_build_grid", "k_associate", "k_vote", "k_normal_equations"]
HOLDS = {"k_organize": "bytes: all of its traffic is algorithmic, at 0.85 of the copy rate of these strides (5.6 TB/s)",
         "k_ring_pick": "the greedy pick's dependent chains; vector and scalar issue both half busy",
         "k_ring_features": "no single unit: 0.78 of the read-stream rate on the bytes it moves, the gather re-reads the ring",
         "k_build_grid": "fabric traffic (the less-flat cloud read 1.12 times + scatter + start tables): time follows bytes in rounds 7 and 8; no CU unit busy",
         "k_associate": "latency of ~5 dependent rounds per query + vector issue; 8 lanes per query in lockstep",
         "k_vote": "vector issue + LDS reads", "k_normal_equations": "latency (one workgroup per scan, f64 chains)"}
# a later round that re-measured the headline only (profiles/r07_bench.json: k_build_grid changed, nothing else): its row comes from there
r7 = last("r07_bench.json")["roofline"] if os.path.exists(os.path.join(P, "r07_bench.json")) and TAG == "r06" else None
# ... and round 8 (profiles/r08_bench.json: k_build_grid and k_ring_pick changed): those two rows come from there
r8 = last("r08_bench.json")["roofline"] if os.path.exists(os.path.join(P, "r08_bench.json")) and TAG == "r06" else None
rows = []
for k in ORDER:
    t = pt["kernels"].get(k, {})
    src = r8 if (r8 and k in ("k_build_grid", "k_ring_pick")) else r7 if (r7 and k == "k_build_grid") else r
    ms, g, i = src["kernel_ms_per_step"][k], src["kernel_algorithmic_GBps"][k], src["issue"].get(k, {})
    if not i and os.path.exists(os.path.join(P, "sq_issue.json")):      # a bench line taken before its counter pass: bench.py's issue model on the pass's counts
        import bench
        q = json.load(open(os.path.join(P, "sq_issue.json")))["kernels"].get(k)
        if q:
            i = {"valu_busy": q["valu"] / (bench.N_SIMD * bench.CLOCK_GHZ * 1e9 / bench.VALU_CYCLES * ms * 1e-3),
                 "salu_busy": q["salu"] / (bench.N_SIMD / 4 * bench.CLOCK_GHZ * 1e9 * ms * 1e-3)}
    traffic = t.get("hbm_read_bytes_per_launch", 0.0) + t.get("hbm_write_bytes_per_launch", 0.0)
    alg = g * 1e9 * ms * 1e-3
    rows.append("| `%s` | %.2f | %.0f (%.3f) | %.2f | %.0f %% / %.0f %% | %s |" % (k, ms, g, g / 8000.0, traffic / alg if alg else 0.0,
                100 * i.get("valu_busy", 0.0), 100 * i.get("salu_busy", 0.0), HOLDS[k]))
dom = r["kernel"]
tok = {
    "DIGEST": pt["source_digest"],
    "S64_KSCANS": "%.1f" % (b["value"] / 1e3), "S64_MS": "%.2f" % b["ms_per_step"],
    "KERNEL_LINE": ", ".join("`%s` %.2f" % (k, km[k]) for k in sorted(km, key=lambda k: -km[k])) + " (round 5: `k_ring_features` 14.72, `k_organize` 13.00, `k_ring_pick` 12.10, `k_associate` 12.10, `k_build_grid` 8.90)",
    "DOM_GBPS": "%.0f" % r["achieved"], "DOM_FRAC": "%.3f" % r["frac"], "DOM_TRAFFIC_GB": "%.1f" % (r["traffic"] / 1e9),
    "DOM_WASTE": "%.2f" % (r["traffic"] / r["algorithmic_bytes_per_launch"]), "DOM_TRAFFIC_TBPS": "%.2f" % (r["traffic_GBps"] / 1e3),
    "DOM_OF_READ": "%.2f" % (r["traffic_GBps"] / 6085.0),
    "WHOLE_FRAC": "%.3f" % r["frac_whole_path"], "WASTE": "%.2f" % r["wasted_traffic"],
    "HDL_KSCANS": "%.1f" % (h["value"] / 1e3), "HDL_ASSOC": "%.2f" % h["roofline"]["kernel_ms_per_step"]["k_associate"],
    "STREAM64": "%.1f" % (st[""]["value"] / 1e3), "STREAM128": "%.1f" % (st["_s128"]["value"] / 1e3),
    "STREAM64_16": "%.1f" % (st["_16_byte_points"]["value"] / 1e3), "STREAM128_16": "%.1f" % (st["_s128_16_byte_points"]["value"] / 1e3),
    "S128_KSCANS": "%.1f" % (s128["value"] / 1e3), "S128_ASSOC": "%.2f" % s128["roofline"]["kernel_ms_per_step"]["k_associate"],
    "S16_KSCANS": "%.0f" % (s16["value"] / 1e3),
    "LATENCY": "registration %.2f ms per 64-ring scan (p90 %.2f), odometry %.2f ms per frame (3 x LM); mapping 0.87 ms per frame (round 5's measurement: that stage is unchanged)"
               % (lat["registration_ms"]["median"], lat["registration_ms"]["p90"], lat["odometry_ms"]["median"]),
    "CPU1": "%.1f" % b["cpu_baseline"]["single_thread"], "CPUALL": "%.0f" % b["cpu_baseline"]["value"], "CPUN": "%d" % b["cpu_baseline"]["cores"],
    "KTABLE": "\n".join(rows),
    "ASSOC_VALU": "%.0f" % (100 * iss["k_associate"]["valu_busy"]), "ASSOC_CAND": "90",
    "ASSOC_WASTE": "%.0f" % ((pt["kernels"]["k_associate"]["hbm_read_bytes_per_launch"] + pt["kernels"]["k_associate"]["hbm_write_bytes_per_launch"]) / (gb["k_associate"] * 1e9 * km["k_associate"] * 1e-3)),
}
parts = ["head.md", "sec2_4.md", "sec5.md", "exact.md", "sec6.md", "sec7.md", "sec8.md", "sec9.md"]
text = "\n".join(open(os.path.join(ROOT, "docs", "_parts", p)).read().rstrip("\n") + "\n" for p in parts)
for k, v in tok.items():
    text = text.replace("@%s@" % k, v)
left = [w for w in text.split("@") if w.isupper() and w.replace("_", "").isalnum() and len(w) > 2]
open(os.path.join(ROOT, "DESIGN.md"), "w").write(text)
print("DESIGN.md written; unfilled tokens:", sorted(set(left)) if left else "none")
