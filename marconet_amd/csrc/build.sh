#!/bin/bash
# Builds libmarconet_hip.so for gfx950 in-tree (the .so travels to the GPU box with the snapshot).
# An object is rebuilt whenever the CONTENT of what it is made from changes: every object carries a stamp (<name>.o.sha) = SHA-256 over its
# source, the shared headers, the compiler flags and the compiler's version string.  (Round 4 keyed on mtimes: a checkout, a `git stash` or a
# copied tree could leave a stale object that linked silently.)  MNET_CLEAN=1 throws everything away first, so that the build PROVES a compile.
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
OUT="$HERE/../lib"
mkdir -p "$OUT"
if [ "${MNET_CLEAN:-0}" != "0" ]; then rm -f "$OUT"/*.o "$OUT"/*.o.tmp "$OUT"/*.o.sha "$OUT"/libmarconet_hip.so "$OUT"/libmarconet_hip.so.sha; echo "[build] MNET_CLEAN: objects removed, full compile"; fi
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
PIDS=()
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function"
SRCS="api conv_igemm conv_igemm_dma conv_dma_swp_gn conv_dma_w4 conv_dma_w4_shuf conv_dma_w4_f32 conv_strip_dma conv_skinny aux_kernels upfold_kernels vit_kernels pack_kernels lq_kernels panel_kernels compare_kernels stitch_kernels page_kernels quad_kernels column_kernels curve_kernels mixed_kernels window_kernels ink_kernels"
# per-source extra flags (conv_dma_swp_gn: see the note at its top; lq_kernels / panel_kernels / page_kernels: their taps must not be contracted, see lq_taps.h / panel_taps.h)
# (curve_kernels: quad_kernels' reason, see curve_map.h; mixed_kernels: page_kernels', quad_kernels' and curve_kernels' reasons together)
# (window_kernels: lq_kernels' reason, it is that kernel on a source with a row pitch)
# (quad_kernels: its fp64 positions must not be contracted either, see quad_map.h; column_kernels: lq_taps.h again, through page_tile.h, which stages the taps for lq_kernels, page_kernels and column_kernels)
extra() { case "$1" in conv_dma_swp_gn) echo "-mllvm -greedy-reverse-local-assignment=1" ;; lq_kernels) echo "-ffp-contract=off" ;; panel_kernels) echo "-ffp-contract=off" ;; page_kernels) echo "-ffp-contract=off" ;; quad_kernels) echo "-ffp-contract=off" ;; column_kernels) echo "-ffp-contract=off" ;; curve_kernels) echo "-ffp-contract=off" ;; mixed_kernels) echo "-ffp-contract=off" ;; window_kernels) echo "-ffp-contract=off" ;; *) echo "" ;; esac; }
HDRS="$HERE/common.h $HERE/conv_args.h $HERE/conv_dma_common.h $HERE/../../include/marconet_hip.h"
CCVER="$("$HIPCC" --version 2>/dev/null | head -3 | tr '\n' ' ')"
stamp() { { cat "$HERE/$1.hip" $HDRS; [ "$1" = conv_dma_swp_gn ] && cat "$HERE/conv_igemm_dma.hip"; [ "$1" = conv_dma_w4_shuf ] && cat "$HERE/conv_dma_w4.hip"; [ "$1" = conv_dma_w4_f32 ] && cat "$HERE/conv_dma_w4.hip"; [ "$1" = lq_kernels ] && cat "$HERE/lq_taps.h" "$HERE/page_tile.h"; [ "$1" = panel_kernels ] && cat "$HERE/panel_taps.h"; [ "$1" = stitch_kernels ] && cat "$HERE/stitch_blend.h"; [ "$1" = upfold_kernels ] && cat "$HERE/../../include/marconet_hip_upfold.h" "$HERE/../../include/marconet_hip_upfold_f32.h"; [ "$1" = page_kernels ] && cat "$HERE/lq_taps.h" "$HERE/page_blend.h" "$HERE/page_tile.h" "$HERE/../../include/marconet_hip_columns.h" "$HERE/cell_paste.h"; [ "$1" = quad_kernels ] && cat "$HERE/quad_map.h" "$HERE/lq_taps.h" "$HERE/page_blend.h" "$HERE/page_tile.h" "$HERE/../../include/marconet_hip_quad.h" "$HERE/warp_paste.h" "$HERE/curve_map.h" "$HERE/../../include/marconet_hip_curve.h"; [ "$1" = column_kernels ] && cat "$HERE/lq_taps.h" "$HERE/page_tile.h" "$HERE/../../include/marconet_hip_columns.h"; [ "$1" = curve_kernels ] && cat "$HERE/curve_map.h" "$HERE/quad_map.h" "$HERE/lq_taps.h" "$HERE/page_blend.h" "$HERE/page_tile.h" "$HERE/../../include/marconet_hip_curve.h" "$HERE/warp_paste.h" "$HERE/../../include/marconet_hip_quad.h"; [ "$1" = mixed_kernels ] && cat "$HERE/cell_paste.h" "$HERE/warp_paste.h" "$HERE/curve_map.h" "$HERE/quad_map.h" "$HERE/lq_taps.h" "$HERE/page_blend.h" "$HERE/page_tile.h" "$HERE/../../include/marconet_hip_columns.h" "$HERE/../../include/marconet_hip_ordered.h" "$HERE/../../include/marconet_hip_quad.h" "$HERE/../../include/marconet_hip_curve.h" "$HERE/../../include/marconet_hip_mixed.h"; [ "$1" = window_kernels ] && cat "$HERE/lq_taps.h" "$HERE/page_tile.h" "$HERE/../../include/marconet_hip_windows.h"; [ "$1" = ink_kernels ] && cat "$HERE/ink.h" "$HERE/../../include/marconet_hip_rowink.h" "$HERE/../../include/marconet_hip_boxink.h" "$HERE/../../include/marconet_hip_skewink.h"; echo "$FLAGS $(extra "$1") ${EXTRA_HIPCC_FLAGS:-} | $CCVER"; } | sha256sum | cut -d' ' -f1; }
for f in $SRCS; do
  want="$(stamp "$f")"
  if [ ! -f "$OUT/$f.o" ] || [ ! -f "$OUT/$f.o.sha" ] || [ "$(cat "$OUT/$f.o.sha")" != "$want" ]; then
    echo "[build] hipcc $f.hip"
    rm -f "$OUT/$f.o.sha"
    ( "$HIPCC" $FLAGS $(extra "$f") ${EXTRA_HIPCC_FLAGS:-} -c "$HERE/$f.hip" -o "$OUT/$f.o.tmp" && mv "$OUT/$f.o.tmp" "$OUT/$f.o" && echo "$want" > "$OUT/$f.o.sha" ) &
    PIDS+=($!)
  fi
done
for p in "${PIDS[@]:-}"; do        # a failed compile must fail the build (a stale object would otherwise be linked)
  if [ -n "$p" ]; then wait "$p"; fi
done
OBJS=""; ALL=""
for f in $SRCS; do OBJS="$OBJS $OUT/$f.o"; ALL="$ALL$(cat "$OUT/$f.o.sha")"; done
LSHA="$(echo "$ALL" | sha256sum | cut -d' ' -f1)"
if [ ! -f "$OUT/libmarconet_hip.so" ] || [ ! -f "$OUT/libmarconet_hip.so.sha" ] || [ "$(cat "$OUT/libmarconet_hip.so.sha")" != "$LSHA" ]; then
  "$HIPCC" --offload-arch=gfx950 -shared -fPIC $OBJS -o "$OUT/libmarconet_hip.so"
  echo "$LSHA" > "$OUT/libmarconet_hip.so.sha"
fi
echo "[build] $OUT/libmarconet_hip.so (sources $LSHA)"
