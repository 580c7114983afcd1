#!/bin/bash
# Builds libiamx.so (gfx950 only) next to the python package.  Cross-compiles without a GPU.
# IAMX_REBUILD=1 ignores the object cache: every source is compiled (what __graft_entry__.build()
# asks for, so that a build check proves the SOURCES build, not that stale objects link).
set -e
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function"
OUT="$HERE/../libiamx.so"
OBJDIR="$HERE/obj"
SRCS="$HERE/common.hip $HERE/match_knn2.hip $HERE/match_knn2v2.hip $HERE/match_knn2sym.hip $HERE/match_post.hip $HERE/host_cleanup.hip $HERE/triangulate.hip $HERE/ba_kernels.hip $HERE/ba_linalg.hip $HERE/ba_schur.hip $HERE/ba_robust.hip $HERE/trf_vec.hip $HERE/comm.hip $HERE/sift.hip $HERE/image_prep.hip $HERE/image_area.hip $HERE/image_colour.hip $HERE/jpeg.hip $HERE/jpeg_entropy.hip $HERE/cache_codec.hip $HERE/surface_grid.hip $HERE/chain_geom.hip $HERE/ortho_raster.hip $HERE/match_verify.hip $HERE/terrain.hip $HERE/match_ratio.hip"
mkdir -p "$OBJDIR"
OBJS=""
for f in $SRCS; do
    o="$OBJDIR/$(basename ${f%.hip}).o"
    if [ -n "$IAMX_REBUILD" ] || [ ! -f "$o" ] || [ "$f" -nt "$o" ] || [ "$HERE/iamx_common.h" -nt "$o" ] || [ "$HERE/jpeg_entropy.h" -nt "$o" ] || [ "$HERE/sym_cand_rule.h" -nt "$o" ] || [ "$HERE/verify_rule.h" -nt "$o" ] || [ "$HERE/five_point.h" -nt "$o" ] || [ "$HERE/../../include/iamx.h" -nt "$o" ]; then
        EXTRA=""
        # the TRF helpers restate numpy expressions: separately rounded multiply and add
        [ "$(basename $f)" = "trf_vec.hip" ] && EXTRA="-ffp-contract=off"
        # the robust loss factors restate numpy expressions (tests/robust_loss_restatement.py), operation by operation
        [ "$(basename $f)" = "ba_robust.hip" ] && EXTRA="-ffp-contract=off"
        # the area downscale restates OpenCV's tap table in doubles, operation by operation
        [ "$(basename $f)" = "image_area.hip" ] && EXTRA="-ffp-contract=off"
        # the radial moments and the fitted mask restate Python's double expressions, operation by operation
        [ "$(basename $f)" = "image_colour.hip" ] && EXTRA="-ffp-contract=off"
        # the surface walk restates scipy's barycentric f64 expressions, operation by operation
        [ "$(basename $f)" = "surface_grid.hip" ] && EXTRA="-ffp-contract=off"
        # the image preparation restates numpy's float32 CLAHE blend and HSV->BGR chains, operation by operation
        [ "$(basename $f)" = "image_prep.hip" ] && EXTRA="-ffp-contract=off"
        # the chain geometry restates numpy / OpenCV double expressions, operation by operation
        [ "$(basename $f)" = "chain_geom.hip" ] && EXTRA="-ffp-contract=off"
        # the orthomosaic's texture coordinate, sample, metric and weight restate numpy's float64 expressions
        [ "$(basename $f)" = "ortho_raster.hip" ] && EXTRA="-ffp-contract=off"
        # the match verification scores and masks with one expression, which must round the same at both sites
        [ "$(basename $f)" = "match_verify.hip" ] && EXTRA="-ffp-contract=off"
        # the terrain look-up and the ray iteration restate scipy's / lib/srtm.py's double expressions, operation by operation
        [ "$(basename $f)" = "terrain.hip" ] && EXTRA="-ffp-contract=off"
        # the ratio bins restate Python's double division and comparisons, operation by operation
        [ "$(basename $f)" = "match_ratio.hip" ] && EXTRA="-ffp-contract=off"
        # the one-wave-per-SIMD sweep (form 2) needs its MFMA
        # accumulators in VGPRs (the allocator's default for > 256 registers is the AGPR half,
        # at a v_accvgpr_read per element the VALU touches)
        [ "$(basename $f)" = "match_knn2sym.hip" ] && EXTRA="-mllvm -amdgpu-mfma-vgpr-form"
        $HIPCC $FLAGS $EXTRA ${IAMX_EXTRA_FLAGS} -c "$f" -o "$o" &
    fi
    OBJS="$OBJS $o"
done
wait
$HIPCC --offload-arch=gfx950 -shared -fPIC -o "$OUT" $OBJS -lz -lpthread
echo "built $OUT"
