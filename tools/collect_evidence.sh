#!/bin/bash
# Round evidence in one go (GPU box; run from the repository root through gpurun):
#   bash tools/collect_evidence.sh [tag]        -> gpurun_out/<tag>_*.{txt,json}   (default tag r6)
# Raw rocprofv3 output goes to /tmp (gpurun merges at most 64 MiB back); the summaries come back
# under gpurun_out/ -- copy the judged ones to profiles/ afterwards (tools/pull_evidence.sh).  Counter passes are separate runs with --pmc only.
TAG="${1:-r6}"
OUT="$PWD/gpurun_out"
REPO="$PWD"
mkdir -p "$OUT"
export TMPDIR=/tmp
SUM="python $REPO/tools/prof_summary.py"
# (counter passes on the 500-image survey: the same kernel instantiation and the same launch
#  shape -- 4096 image pairs of 4096 x 4096 rows per launch -- as the 2812-image headline, 31
#  launches instead of 965; rocprofv3 --pmc segfaults inside the 2812-image run on this pool's
#  image, 6 s in, before the first sweep: profiles/r6_pmc_2812_segfault.txt)
BENCH_PMC="python $REPO/bench.py --images 500 --steps 1 --warmup 0 --no-ba --no-sift --no-cpu-baseline --verify-pairs 0 --no-e2e --no-survey"
# BA + SIFT kernels (a small matching section in front of them)
AUX_PMC="python $REPO/bench.py --full --images 64 --steps 1 --warmup 0 --no-cpu-baseline --verify-pairs 0 --no-e2e --no-sift-full --no-survey"

step() { echo "== $1 ($(date +%T))"; }
# The instantiation the library launches: every summary below must name it, or the run fails
# (round 3 shipped a kernel swapped in after the last evidence pass).
export IAMX_EXPECT_KERNEL="$(python -c 'from imageanalysis_amd import kernels; print(kernels.lib().iamx_knn2sym_kernel_id(2).decode())')"
echo "shipped sweep: $IAMX_EXPECT_KERNEL"
check_kernel() {   # $1 = summary file that has to contain the launched template string
    if ! grep -qF "$IAMX_EXPECT_KERNEL" "$1"; then
        echo "EVIDENCE MISMATCH: $1 does not mention $IAMX_EXPECT_KERNEL"; FAILED=1
    fi
}
FAILED=0

if [ "${STAGE:-AB}" != "B" ]; then
if [ -z "$NO_TESTS" ]; then
step "gpu tests"
timeout 1500 python -m pytest tests -m gpu -q > "$OUT/${TAG}_gpu_tests.txt" 2>&1
tail -n 3 "$OUT/${TAG}_gpu_tests.txt"
fi

step "PMC: HBM traffic of the matching step (FETCH_SIZE, WRITE_SIZE: separate passes)"
for C in FETCH_SIZE WRITE_SIZE; do
    # (a counter pass of this command takes ~20 s; one WRITE_SIZE pass of round 6 hung until its limit,
    #  then 1200 s: a hung pass is retried once under a short limit)
    (cd /tmp && { timeout 300 rocprofv3 --pmc $C --output-format csv -d /tmp/p_$C -o b -- $BENCH_PMC > /dev/null 2> /tmp/p_$C.err || { rm -rf /tmp/p_$C; timeout 300 rocprofv3 --pmc $C --output-format csv -d /tmp/p_$C -o b -- $BENCH_PMC > /dev/null 2> /tmp/p_$C.err; }; })
    lc=$(echo $C | tr 'A-Z' 'a-z' | sed 's/_size//')
    $SUM /tmp/p_$C "$OUT/${TAG}_knn2sym_pmc_${lc}.txt" > /dev/null
done
if [ -z "$NO_AUX" ]; then
step "PMC: HBM traffic of the BA and SIFT kernels (FETCH_SIZE, WRITE_SIZE: separate passes)"
for C in FETCH_SIZE WRITE_SIZE; do
    (cd /tmp && timeout 420 rocprofv3 --pmc $C --output-format csv -d /tmp/a_$C -o b -- $AUX_PMC > /dev/null 2> /tmp/a_$C.err)
    lc=$(echo $C | tr 'A-Z' 'a-z' | sed 's/_size//')
    $SUM /tmp/a_$C "$OUT/${TAG}_aux_pmc_${lc}.txt" > /dev/null
    cp "$OUT/${TAG}_aux_pmc_${lc}.txt" "$REPO/profiles/${TAG}_aux_pmc_${lc}.txt"
done
python "$REPO/tools/aux_traffic_json.py" "$TAG" && cp "$REPO/profiles/${TAG}_ba_sift_traffic.json" "$OUT/"
fi
step "PMC: SQ / MFMA busy"
(cd /tmp && timeout 420 rocprofv3 --pmc GRBM_GUI_ACTIVE SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_VALU_MFMA_BUSY_CYCLES \
    SQ_INSTS_VALU_MFMA_MOPS_I8 SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_WAIT_INST_LDS \
    --output-format csv -d /tmp/p_sq -o b -- $BENCH_PMC > /dev/null 2> /tmp/p_sq.err)
$SUM /tmp/p_sq "$OUT/${TAG}_knn2sym_pmc_sq.txt" > /dev/null
head -12 "$OUT/${TAG}_knn2sym_pmc_sq.txt" | cut -c1-140

step "traffic summaries -> profiles/ (what bench.py quotes)"
for f in knn2sym_pmc_fetch knn2sym_pmc_write knn2sym_pmc_sq; do
    cp "$OUT/${TAG}_$f.txt" "$REPO/profiles/${TAG}_$f.txt"
done
for f in knn2sym_pmc_fetch knn2sym_pmc_write knn2sym_pmc_sq; do check_kernel "$REPO/profiles/${TAG}_$f.txt"; done
python "$REPO/tools/update_traffic_json.py" "$TAG" || FAILED=1
[ -f "$REPO/profiles/${TAG}_knn2sym_traffic.json" ] && cp "$REPO/profiles/${TAG}_knn2sym_traffic.json" "$OUT/"

step "bench"
timeout 1500 python bench.py --full --steps 20 --warmup 5 > "$OUT/${TAG}_bench_latest.json" 2> "$OUT/${TAG}_bench_latest.err"
tail -c 600 "$OUT/${TAG}_bench_latest.json"; echo

fi
if [ "${STAGE:-AB}" != "A" ]; then
step "kernel stats of the bench command"
(cd /tmp && timeout 1500 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/p_stats -o b -- \
    python "$REPO/bench.py" --full --steps 2 --warmup 1 --no-cpu-baseline --no-e2e --no-survey > "$OUT/${TAG}_bench_under_rocprof.json" 2> /tmp/p_stats.err)
$SUM /tmp/p_stats "$OUT/${TAG}_kernel_stats.txt" > /dev/null
python "$REPO/tools/prof_gaps.py" /tmp/p_stats lsmr > "$OUT/${TAG}_lsmr_gaps.txt" 2>&1
head -8 "$OUT/${TAG}_kernel_stats.txt" | cut -c1-160
check_kernel "$OUT/${TAG}_kernel_stats.txt"
cp "$OUT/${TAG}_kernel_stats.txt" "$REPO/profiles/${TAG}_kernel_stats.txt"

step "SIFT kernel stats"
(cd /tmp && timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/p_sift -o s -- \
    python "$REPO/tools/sift_time.py" 0.4 > "$OUT/${TAG}_sift_time.txt" 2>&1)
$SUM /tmp/p_sift "$OUT/${TAG}_sift_kernel_stats.txt" > /dev/null
cp "$OUT/${TAG}_sift_kernel_stats.txt" "$OUT/${TAG}_sift_time.txt" "$REPO/profiles/"

if [ -z "$NO_ENTRY" ]; then
step "entry points"
timeout 600 python tools/find_matches_rate.py > "$OUT/${TAG}_fm_dense.txt" 2>&1; tail -n 1 "$OUT/${TAG}_fm_dense.txt"
timeout 900 python tools/detect_rate.py 192 --no-serial > "$OUT/${TAG}_detect_rate_final.txt" 2>&1; tail -n 4 "$OUT/${TAG}_detect_rate_final.txt"
# configs[2] through matcher.find_matches (2812 x 4096, 3.95 M pairs)
timeout 600 python tools/find_matches_rate.py 38 74 4096 > "$OUT/${TAG}_fm_config2_run.txt" 2>&1; tail -n 3 "$OUT/${TAG}_fm_config2_run.txt"
# configs[4] at 512 rendered 20 MP frames (what bench.py quotes as e2e_full_recorded)
IAMX_LINK_TIMING=1 timeout 900 python bench.py --steps 1 --warmup 0 --no-ba --no-sift --no-cpu-baseline --verify-pairs 0 --no-e2e --no-survey \
    --images 64 --e2e-full 512 > "$OUT/${TAG}_e2e_full_run.json" 2> "$OUT/${TAG}_e2e_full_run.err"
grep iamx_link_matches "$OUT/${TAG}_e2e_full_run.err" > "$OUT/${TAG}_link_passes_512.txt"
python - "$OUT/${TAG}_e2e_full_run.json" "$OUT/${TAG}_e2e_full_512.json" <<'PY'
import json, sys
rec = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]).get("e2e_full")
if rec:
    json.dump(rec, open(sys.argv[2], "w"), indent=1)
    print("e2e_full:", rec.get("images"), "frames,", rec.get("seconds_total", rec.get("seconds")), "s")
PY
fi
fi
step "done"
[ "$FAILED" = 0 ] || { echo "collect_evidence: FAILED (kernel mismatch)"; exit 1; }
