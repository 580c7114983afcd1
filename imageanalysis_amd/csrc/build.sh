#!/bin/bash
# Builds libiamx.so (gfx950 only) next to the python package, from every csrc/*.hip.  Cross-compiles
# without a GPU.  An object in obj/ is reused unless its source, any csrc/*.h or include/iamx.h is newer;
# IAMX_REBUILD=1 ignores that cache and compiles every source (what __graft_entry__.build() asks for).
# A source that does not compile fails the build: nothing is linked and libiamx.so is removed, so that
# no library older than its sources is left to load.
#   build.sh --flags <name>.hip   prints the flags <name>.hip is compiled with and compiles nothing
#                                 (the one place the tests that read device assembly learn them from)
#   HIPCC, IAMX_EXTRA_FLAGS       the compiler; flags appended to every compile
#   MAX_JOBS                      compiles running at a time (default and ceiling: 16)
set -e
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function"
HEADER="$HERE/../../include/iamx.h"
OUT="$HERE/../libiamx.so"
OBJDIR="$HERE/obj"

# every flag of one source: the common ones, its own, the caller's
flags_of() {
    local extra=""
    case "$(basename "$1")" in
        # the TRF helpers restate numpy expressions: separately rounded multiply and add
        trf_vec.hip) extra="-ffp-contract=off" ;;
        # the robust loss factors restate numpy expressions (tests/robust_loss_restatement.py), operation by operation
        ba_robust.hip) extra="-ffp-contract=off" ;;
        # the area downscale restates OpenCV's tap table in doubles, operation by operation
        image_area.hip) extra="-ffp-contract=off" ;;
        # the radial moments and the fitted mask restate Python's double expressions, operation by operation
        image_colour.hip) extra="-ffp-contract=off" ;;
        # the surface walk restates scipy's barycentric f64 expressions, operation by operation
        surface_grid.hip) extra="-ffp-contract=off" ;;
        # the image preparation restates numpy's float32 CLAHE blend and HSV->BGR chains, operation by operation
        image_prep.hip) extra="-ffp-contract=off" ;;
        # the chain geometry restates numpy / OpenCV double expressions, operation by operation
        chain_geom.hip) extra="-ffp-contract=off" ;;
        # the orthomosaic's texture coordinate, sample, metric and weight restate numpy's float64 expressions
        ortho_raster.hip) extra="-ffp-contract=off" ;;
        # the match verification scores and masks with one expression, which must round the same at both sites
        match_verify.hip) extra="-ffp-contract=off" ;;
        # the terrain look-up and the ray iteration restate scipy's / lib/srtm.py's double expressions, operation by operation
        terrain.hip) extra="-ffp-contract=off" ;;
        # the ratio bins restate Python's double division and comparisons, operation by operation
        match_ratio.hip) extra="-ffp-contract=off" ;;
        # the one-wave-per-SIMD sweep (form 2) needs its MFMA
        # accumulators in VGPRs (the allocator's default for > 256 registers is the AGPR half,
        # at a v_accvgpr_read per element the VALU touches)
        match_knn2sym.hip) extra="-mllvm -amdgpu-mfma-vgpr-form" ;;
    esac
    echo $FLAGS $extra ${IAMX_EXTRA_FLAGS}
}

if [ "$1" = "--flags" ]; then
    [ -f "$HERE/$2" ] || { echo "build.sh --flags: no source $HERE/$2" >&2; exit 2; }
    flags_of "$2"
    exit 0
fi

JOBS="${MAX_JOBS:-16}"
case "$JOBS" in ''|*[!0-9]*) JOBS=16 ;; esac
[ "$JOBS" -gt 16 ] && JOBS=16
[ "$JOBS" -lt 1 ] && JOBS=1

# sorted, the two that compile longest moved to the front of the queue
SRCS=("$HERE/match_knn2sym.hip" "$HERE/sift.hip")
for f in "$HERE"/*.hip; do
    case "$(basename "$f")" in match_knn2sym.hip|sift.hip) ;; *) SRCS+=("$f") ;; esac
done

stale() {   # source, object
    local dep
    [ -n "$IAMX_REBUILD" ] || [ ! -f "$2" ] && return 0
    for dep in "$1" "$HERE"/*.h "$HEADER"; do
        [ "$dep" -nt "$2" ] && return 0
    done
    return 1
}

mkdir -p "$OBJDIR"
OBJS=() PIDS=() STARTED=()
running=0
for f in "${SRCS[@]}"; do
    o="$OBJDIR/$(basename "${f%.hip}").o"
    OBJS+=("$o")
    stale "$f" "$o" || continue
    if [ "$running" -ge "$JOBS" ]; then
        wait -n || true             # any one job; its status is read by pid below
        running=$((running - 1))
    fi
    rm -f "$o"                      # a failed compile leaves no object of an earlier one behind
    "$HIPCC" $(flags_of "$f") -c "$f" -o "$o" &
    PIDS+=($!) STARTED+=("$f")
    running=$((running + 1))
done
FAILED=()
for i in "${!PIDS[@]}"; do
    wait "${PIDS[$i]}" || FAILED+=("$(basename "${STARTED[$i]}")")
done
if [ "${#FAILED[@]}" -gt 0 ]; then
    for f in "${FAILED[@]}"; do rm -f "$OBJDIR/${f%.hip}.o"; done
    rm -f "$OUT"
    echo "build.sh: did not compile: ${FAILED[*]} -- nothing linked, $OUT removed" >&2
    exit 1
fi
TMP="$HERE/../libiamx.tmp.$$.so"
"$HIPCC" --offload-arch=gfx950 -shared -fPIC -o "$TMP" "${OBJS[@]}" -lz -lpthread || { rm -f "$TMP" "$OUT"; exit 1; }
mv -f "$TMP" "$OUT"
echo "built $OUT"
