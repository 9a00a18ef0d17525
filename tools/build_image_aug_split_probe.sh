#!/bin/bash
# builds tools/bin/libimage_aug_split.so (gfx950): csrc/vl_image_augment.hip with the launch-per-op baseline beside it
set -e
cd "$(dirname "$0")/.."
mkdir -p tools/bin
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -Wno-unused-result -Iinclude -Ivit-lens_amd/csrc \
  -x hip tools/image_aug_split_probe.hip -o tools/bin/libimage_aug_split.so
