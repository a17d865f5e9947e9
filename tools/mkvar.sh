# Build a variant of libhiphuff.so with extra compile flags for same-box A/B
# (tools/gpu_ab.sh): bash tools/mkvar.sh NAME "-DFOO=1 ..." -> build/var/NAME.so
# (`make variant`, which knows the library's units; its result moved there)
set -e
cd "$(dirname "$0")/.."
N=$1; shift
make -j8 variant V="$N" HIPEXTRA="$*"
mkdir -p build/var
mv "build/libhiphuff_$N.so" "build/var/$N.so"
echo "build/var/$N.so"
