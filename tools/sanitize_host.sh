#!/bin/bash
# AddressSanitizer + UndefinedBehaviorSanitizer over the HOST side of the library (CPU only: GPU ASan is
# not available on this pool): every host unit of btl_bloomfilter_amd/build.py (HOST_UNITS: the C ABI's planning, file
# headers and argument checks, the FASTA/FASTQ parser and its reader threads) is rebuilt instrumented and linked with
# the kernel objects as built; then the CPU test cases that drive them run against that library.
#     tools/sanitize_host.sh            (from the repository root)
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd "$ROOT"
python3 -m btl_bloomfilter_amd.build > /dev/null
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
SAN="-fsanitize=address,undefined -fno-gpu-sanitize -fno-omit-frame-pointer -g -O1"
P=btl_bloomfilter_amd
mkdir -p $P/_build_asan
HOST_UNITS=$(python3 -c "from btl_bloomfilter_amd import build as b; print(' '.join(b.HOST_UNITS))")
KERNEL_OBJS=$(python3 -c "from btl_bloomfilter_amd import build as b; print(' '.join('$P/_build/%s.o' % n for n, _, _ in b.UNITS if n not in b.HOST_UNITS))")
HOST_OBJS=
for u in $HOST_UNITS; do
	(set -x; $HIPCC --offload-arch=gfx950 -std=c++17 -fPIC -Wall -Wno-unused-function $SAN -c -o $P/_build_asan/$u.o $P/csrc/$u.cpp)
	HOST_OBJS="$HOST_OBJS $P/_build_asan/$u.o"
done
$HIPCC --offload-arch=gfx950 -shared -fPIC $SAN -o $P/libbtlbf_asan.so $HOST_OBJS $KERNEL_OBJS -lz
RT=$(/opt/rocm/lib/llvm/bin/clang -print-file-name=libclang_rt.asan-x86_64.so)
[ -f "$RT" ] || RT=$(/opt/rocm/lib/llvm/bin/clang --print-file-name=libclang_rt.asan.so)
echo "runtime: $RT"
LD_PRELOAD=$RT ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 \
	BTLBF_LIB=$ROOT/$P/libbtlbf_asan.so python3 -m pytest tests/test_fastx.py tests/test_abi_cpu.py -q -m "not gpu" -p no:cacheprovider
# the test-only reference miBF driver (oracle/ref_mibf_driver.cpp over oracle/standin/), instrumented the same way, under
# the test that drives it -- only where the reference tree is there to build it from.  (tests/test_oracle_vs_ref.py is
# not run this way: its raw k-mer case calls the reference where it reads past its own 2-/3-mer tables.)
if make -C oracle _ref/libbtlref_asan.so > /dev/null 2>&1; then
	LD_PRELOAD=$RT ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 \
		BTLBF_REF_SO=$ROOT/oracle/_ref/libbtlref_asan.so python3 -m pytest tests/test_mibf_vs_ref.py -q -m "not gpu" -p no:cacheprovider
else
	echo "reference driver: not built here (no reference tree), skipped"
fi
