"""Build libdgx.so (all HIP kernels + the C ABI of include/divergen_hip.h) for gfx950.

    python -m divergen_amd.csrc.build        # or __graft_entry__.build()
    DGX_DEV=1 python -m divergen_amd.csrc.build      # the development library, see build(dev=True)

hipcc cross-compiles without a GPU.  The .so is built IN-TREE (divergen_amd/csrc/libdgx.so) so it
travels with the repo snapshot to the GPU box; it is git-ignored.
Flags: -ffp-contract=off keeps the fp32 op sequence of the index-producing kernels identical to the
CPU oracle (bit-exact RoI geometry / NMS / targets); -munsafe-fp-atomics selects the hardware fp32
atomic add for the ROIAlign / bias-table gradient scatters.
"""
import glob
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCES = ["window_attention.hip", "window_shuffle.hip", "roi_align.hip", "nms_boxes.hip",
           "centernet_targets.hip", "compositor.hip", "poisson_blend.hip", "self_copy.hip", "remove_background.hip", "polygon_raster.hip", "resize_u8.hip", "optim.hip", "im2col.hip", "wgrad256.hip", "gemm_nt.hip", "gemm_lw.hip", "gemm_k192.hip", "wgrad_lw.hip", "transpose.hip", "prof.hip", "preprocess.hip", "mask_loss.hip", "layernorm.hip", "l2norm.hip", "residual.hip", "colsum.hip", "groupnorm.hip", "gelu.hip", "detic_loss.hip", "dyn_vocab.hip", "text_encoder.hip", "centernet_loss.hip", "cascade_refine.hip", "image_label.hip", "wsddn_loss.hip", "caption_loss.hip", "mask_paste.hip", "lvis_eval.hip", "grad_bank.hip", "roi_sample.hip", "centernet_decode.hip", "topk_sort.hip", "resnet_ops.hip", "abi.hip"]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
         "-munsafe-fp-atomics", "-Wno-unused-result"]


def build(verbose=False, force=False, dev=False):
    """dev: the development build (-DDGX_DEV: the phase clocks of dev_clock.h compiled in).  Its objects and its library live apart
    from the product's (_obj/dev/libdgx_dev.so, selected with DGX_LIB of _lib.py): neither build ever links an object of the other."""
    flags = FLAGS + (["-DDGX_DEV"] if dev else [])
    obj_dir = os.path.join(HERE, "_obj", "dev") if dev else os.path.join(HERE, "_obj")
    out = os.path.join(obj_dir, "libdgx_dev.so") if dev else os.path.join(HERE, "libdgx.so")
    srcs = [os.path.join(HERE, s) for s in SOURCES if os.path.exists(os.path.join(HERE, s))]
    hdrs = glob.glob(os.path.join(HERE, "*.h")) + [os.path.join(HERE, "..", "..", "include", "divergen_hip.h")]
    objs = []
    os.makedirs(obj_dir, exist_ok=True)
    procs = []
    for s in srcs:
        o = os.path.join(obj_dir, os.path.basename(s) + ".o")
        objs.append(o)
        if force or not os.path.exists(o) or any(os.path.getmtime(d) > os.path.getmtime(o) for d in [s] + hdrs):
            cmd = [HIPCC] + flags + ["-c", s, "-o", o]
            if verbose:
                print(" ".join(cmd))
            procs.append((s, subprocess.Popen(cmd)))
    for s, p in procs:
        if p.wait() != 0:
            raise RuntimeError("hipcc failed on %s" % s)
    if force or procs or not os.path.exists(out):
        cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out] + objs
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    return out


if __name__ == "__main__":
    print(build(verbose=True, force="--force" in sys.argv, dev=os.environ.get("DGX_DEV") == "1"))
