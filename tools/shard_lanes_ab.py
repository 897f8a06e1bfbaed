"""The 8- / 4-frame per-rank shards of cfg3 as whole pipelined steps with 2 or 3 copies of the network at 4 frames (bench.SHARD_LANES_4): python tools/shard_lanes_ab.py"""
import sys, json, os, subprocess, tempfile
legs = os.path.join(tempfile.mkdtemp(), "legs.json")
for n in (2, 3):
    code = f"import bench,sys; bench.SHARD_LANES_4={n}; sys.argv=['bench.py','--full','--no-cpu-baseline','--no-alt-precisions','--no-h2d-leg','--legs-file',{legs!r}]; bench.main()"
    subprocess.run([sys.executable, "-c", code], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    d = json.load(open(legs))
    print("lanes at 4 frames:", n, {k: (round(v["value"]), round(v["two_streams"]["value"]), v["two_streams"].get("copies")) for k, v in d["strong_scaling_shards"].items() if isinstance(v, dict) and "two_streams" in v}, flush=True)
