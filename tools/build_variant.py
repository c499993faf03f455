#!/usr/bin/env python3
"""Build a variant of libpbrt_hip.so next to the product library for A/B measurements in ONE gpurun call.

    python tools/build_variant.py NAME [-DKNOB=V ...] [--mllvm OPT ...] [--units rt_trace.hip,rt_mega_p.hip]

compiles the listed translation units (default: all) with the extra defines into pbrt-v1_amd/lib/obj_NAME/, takes the others
from the product build (pbrt-v1_amd/lib/obj/), and links pbrt-v1_amd/lib/libpbrt_hip_NAME.so.  A process picks it with
PBRT_HIP_LIB_PATH=<that file> (read by pbrt-v1_amd/__init__.py only when PBRT_HIP_TUNE is set, like every other knob).
The work is the package's build_variant(name, defines), which compiles only what changed since the last call."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry


def main():
    pkg = entry.load_package()
    name = sys.argv[1]
    defines = [a for a in sys.argv[2:] if a.startswith("-D")]
    arch, units = None, None
    for i, a in enumerate(sys.argv):
        if a == "--mllvm":                                        # a code generation option for the device compiler (scheduling experiments)
            defines += ["-mllvm", sys.argv[i + 1]]
        if a == "--arch":                                         # --arch gfx950:xnack- : another target id for the device code (code generation experiments)
            arch = sys.argv[i + 1]
        if a == "--units":
            units = sys.argv[i + 1].split(",")
    print(pkg.build_variant(name, defines, units=units, arch=arch))


if __name__ == "__main__":
    main()
