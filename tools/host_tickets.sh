#!/bin/bash
# Host-side sanitizer runs of the conversion tickets (CPU container only; nothing of the kind goes to a GPU): builds the host
# pass against tools/hipstub and runs tools/host_tickets_driver.py on it with the sanitizer's shared runtime preloaded.
#   tools/host_tickets.sh asan    AddressSanitizer + UBSan (make host-asan)
#   tools/host_tickets.sh tsan    ThreadSanitizer (make host-tsan)
set -e
cd "$(dirname "$0")/.."
MODE=${1:-asan}
make -j8 host-$MODE > /dev/null
RT=$(/opt/rocm/lib/llvm/bin/clang++ -print-file-name=libclang_rt.$MODE-x86_64.so)
if [ "$MODE" = tsan ]; then
  # the interpreter is not TSan-clean: tools/tsan.supp silences reports whose frames all lie outside librvcx, nothing else
  exec env LD_PRELOAD="$RT" TSAN_OPTIONS="halt_on_error=1:exitcode=66:suppressions=$PWD/tools/tsan.supp:report_signal_unsafe=0" \
      RVCX_LIBRARY="$PWD/build/tsan/librvcx_tsan.so" RVCX_DEBUG=1 python3 tools/host_tickets_driver.py
fi
exec env LD_PRELOAD="$RT" ASAN_OPTIONS=detect_leaks=0:abort_on_error=1:halt_on_error=1 \
    UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 RVCX_LIBRARY="$PWD/build/asan/librvcx_asan.so" RVCX_DEBUG=1 \
    python3 tools/host_tickets_driver.py
