# final tree of round 5: GPU suite, smoke, bench lines of all four workloads (the kernels are those of profiles/r05_kernel_stats_*)
R=$(cd "$(dirname "$0")/.." && pwd); OUT=${OUT:-$R/prof_out}; mkdir -p "$OUT"; export OUT; cd $R
timeout 1500 python -m pytest tests -m gpu -q 2>&1 | tail -4
python -c "import __graft_entry__ as g; g.smoke()"
T0=$(date +%s); timeout 900 python bench.py --full > $OUT/bench_default.json 2> $OUT/bench_default.err; echo "default bench.py --full: rc=$? $(( $(date +%s) - T0 )) s"
timeout 900 python bench.py --full --steps 20 --warmup 3 > $OUT/bench_final.json 2> $OUT/bench_final.err; echo rc=$?
rm -f $OUT/bench_configs.jsonl $OUT/bench_configs.err
for w in c2 c4 c5; do S=10; [ $w = c5 ] && S=5; timeout 900 python bench.py --workload $w --full --steps $S --no-ntt >> $OUT/bench_configs.jsonl 2>> $OUT/bench_configs.err; done
python - <<'P'
import json, os
d=json.load(open(os.path.join(os.environ["OUT"], "bench_final.json")))
print("c3", d["value"], d["verified"], d.get("accounting_problems"))
cb=d["concurrent_b1"]; print({k:cb[k] for k in cb if k in ("K","coalesced","coalesced_sync_each","deferred","deferred_sync_each","verified")})
for r in cb.get("compiled_host",[]): print({k:r.get(k) for k in ("K","sync_each","deferred_depth","mean_batch","ops_per_s","verified_callers","error")})
for l in open(os.path.join(os.environ["OUT"], "bench_configs.jsonl")):
    d=json.loads(l); print(d["config"]["workload"][:30], d["value"], d.get("verified"), d.get("accounting_problems"))
    cb=d.get("concurrent_b1") or {}
    for r in cb.get("compiled_host",[]): print("   ", {k:r.get(k) for k in ("K","sync_each","coalescing","max_batch","deferred_depth","mean_batch","ops_per_s","verified_callers","error")})
    if "deferred" in cb: print("   ", {k:cb[k] for k in cb if k in ("K","coalesced","deferred","deferred_sync_each","lone_caller","uncoalesced_K4","verified","error")})
P
