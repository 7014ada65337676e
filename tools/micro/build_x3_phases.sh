#!/bin/bash
# libfgn_hip.so with the phase clocks of conv_pw_x3_kernel compiled in (-DX3_PHASES) and the kernel instances that were
# measured and not chosen (-DFGN_EXPERIMENTS): tools/micro/libfgn_hip_x3ph.so (and libfgn_hip_h2ph.so for conv_pw_h2_kernel),
# loaded by tools/x3_probe.py --phases through FGN_HIP_LIB.
set -euo pipefail
cd "$(dirname "$0")/../.."
F="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -DX3_PHASES -DFGN_EXPERIMENTS -mllvm -amdgpu-atomic-optimizer-strategy=None -Wno-unused-function -Wno-inline-asm"
hipcc $F -c fgn_amd/csrc/conv_igemm.hip -o /tmp/conv_igemm_x3ph.o
objs=/tmp/conv_igemm_x3ph.o
for f in abi spatial norm winograd relation rpn_post det_post mask train train_bwd optim; do
  [ -f fgn_amd/csrc/$f.o ] || python -m fgn_amd.build
  objs="$objs fgn_amd/csrc/$f.o"
done
hipcc --offload-arch=gfx950 -shared -fPIC -o tools/micro/libfgn_hip_x3ph.so $objs
echo built tools/micro/libfgn_hip_x3ph.so
# the same for conv_pw_h2_kernel (-DH2_PHASES, conv_pw_h2.h): tools/micro/libfgn_hip_h2ph.so
hipcc ${F/-DX3_PHASES/-DH2_PHASES} -c fgn_amd/csrc/conv_igemm.hip -o /tmp/conv_igemm_h2ph.o
hipcc --offload-arch=gfx950 -shared -fPIC -o tools/micro/libfgn_hip_h2ph.so /tmp/conv_igemm_h2ph.o ${objs#/tmp/conv_igemm_x3ph.o}
echo built tools/micro/libfgn_hip_h2ph.so
# ... and with the epilogue in its pass-per-wave-row form on every instance (-DH2_EPILOGUE_PASSES: what the one-K-group
# instances ran before the wave-private epilogue), for the epilogue's phase split of both forms under the same stamps:
# tools/micro/libfgn_hip_h2ph_passes.so (tools/x3_probe.py --phases --epilogue)
hipcc ${F/-DX3_PHASES/-DH2_PHASES -DH2_EPILOGUE_PASSES} -c fgn_amd/csrc/conv_igemm.hip -o /tmp/conv_igemm_h2ph_passes.o
hipcc --offload-arch=gfx950 -shared -fPIC -o tools/micro/libfgn_hip_h2ph_passes.so /tmp/conv_igemm_h2ph_passes.o ${objs#/tmp/conv_igemm_x3ph.o}
echo built tools/micro/libfgn_hip_h2ph_passes.so
