"""Teeth segmentation (csrc/teeth.hip): 256 seeded 512 x 512 frames through TeethSegmenter.mask, beside teeth_torch on the
same GPU and the fp32 statement on the CPU (scripts/_bench_frames.py has the method).

    python scripts/bench_teeth.py [--json out.json] [--frames 256] [--batch 8]
"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bench_frames
from instag_amd import teeth as T

if __name__ == "__main__":
    _bench_frames.main(T, T.FPNWeights.random(0), T.TeethSegmenter, lambda seg, frames: seg.mask(frames), T.teeth_torch,
                       extra=lambda got: dict(teeth_share=float(got.double().mean())))
