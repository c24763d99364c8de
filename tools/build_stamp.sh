# diagnostic libraries of the persistent trunk kernel (never shipped, never loaded by the product):
#   tools/debug/libacimg_stamp.so   in-kernel cycle stamps (+ the ablation switches)   -> tools/stamp_probe.py
#   tools/debug/libacimg_ablate.so  the ablation switches alone, undisturbed timing    -> tools/ablate_probe.py
# Built through csrc/Makefile (its sources, its flags) with the define, into a directory of their own.
set -e
cd "$(dirname "$0")/../acoustic-image-generation_amd/csrc"
OUT=../../tools/debug
for kind in stamp ablate; do
  DEF=$([ $kind = stamp ] && echo -DACIMG_STAMP || echo -DACIMG_ABLATE)
  make -j4 OUT=$OUT/$kind LIB=libacimg_$kind.so DEFS=$DEF
  mv $OUT/$kind/libacimg_$kind.so $OUT/
  rm -rf $OUT/$kind
  echo built $OUT/libacimg_$kind.so
done
