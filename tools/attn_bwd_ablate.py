"""Diagnostic: where does token_attn_bwd_kernel spend its time?  Builds variants of token_attn_train_f32.hip with phases removed
(-DLIME_ATTN_BWD_ABLATE=mask: 1 no global staging, 2 no S / dP MFMAs, 4 no softmax, 8 no dV, 16 no dQ / dK, 32 no stores) and
times the body (S = 128) and title (S = 32) shapes.  64: the S / dP MFMAs run on register operands (no K / V fragment reads).
Every variant is a whole library; the split product is switched off so that token_attn_bwd_kernel takes both shapes.

    python tools/attn_bwd_ablate.py
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from lime_cikm25_amd import _lib, ops  # noqa: E402
from lime_cikm25_amd import build as lime_build  # noqa: E402

MASKS = [0, 2, 64, 4 | 8 | 16, 4 | 8 | 16 | 64, 2 | 4 | 8 | 16]


def build(mask):
    so = os.path.join(ROOT, 'tools', 'probes', 'liblime_attn_bwd_%d.so' % mask)
    src = os.path.join(ROOT, 'lime_cikm25_amd', 'csrc')
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(os.path.join(src, 'token_attn_train_f32.hip')):
        subprocess.run(['hipcc', '-O3', '-std=c++17', '--offload-arch=gfx950', '-fPIC', '-shared',
                        '-DLIME_ATTN_BWD_ABLATE=%d' % mask, '-o', so] + lime_build.sources(), check=True)
    return so


def main():
    dev = 'cuda'
    nh, hd, hs = 10, 30, 32
    W = nh * hs
    for mask in MASKS:
        _lib.LIB_PATH, _lib._lib = build(mask), None          # the wrappers below call this variant
        _lib.load().lime_set_split_gemm(0)
        line = 'mask %2d' % mask
        for n_seq, S in ((1760, 128), (1760, 32)):
            tok = n_seq * S
            qkv = (torch.rand(tok, 3 * W, device=dev) - 0.5)
            dout = torch.rand(tok, nh * hd, device=dev) - 0.5
            dqkv = torch.empty_like(qkv)

            def run():
                ops.token_attention_bwd(qkv[:, :W], qkv[:, W:2 * W], qkv[:, 2 * W:], dout, n_seq, S, nh, hd, 1.0 / hd ** 0.5, head_stride=hs,
                                        dqkv=dqkv)
            for _ in range(3):
                run()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                run()
            e1.record()
            torch.cuda.synchronize()
            line += '   S=%3d %7.1f us' % (S, e0.elapsed_time(e1) * 100)
        print(line, flush=True)


if __name__ == '__main__':
    main()
