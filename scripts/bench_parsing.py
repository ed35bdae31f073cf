"""Face parsing (csrc/parsing.hip): 256 seeded 512 x 512 frames through FaceParser.parse, beside parse_torch on the same
GPU and the fp32 statement on the CPU (scripts/_bench_frames.py has the method).

    python scripts/bench_parsing.py [--json out.json] [--frames 256] [--batch 8]
"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bench_frames
from instag_amd import parsing as P

if __name__ == "__main__":
    _bench_frames.main(P, P.BiSeNetWeights.random(0), P.FaceParser, lambda parser, frames: parser.parse(frames), P.parse_torch)
