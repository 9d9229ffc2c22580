"""CPU: what bsgs_mi355x -kangaroo -infile refuses at the command line, before any device is looked for."""
import os
import subprocess

from pybsgs.ecpy import mul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "bsgs-cuda_amd", "build", "bsgs_mi355x")


def compressed(p):
    return "%02x%064x" % (2 + (p[1] & 1), p[0])


def run(args, cwd):
    if not os.path.exists(HOST):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "bsgs-cuda_amd"), "-s"])
    return subprocess.run([HOST, "-kangaroo", "-dir", str(cwd)] + args, capture_output=True, text=True, timeout=120)


def test_refusals_without_a_gpu(tmp_path):
    keys = tmp_path / "keys.txt"
    keys.write_text("\n".join(compressed(mul((1 << 40) + 7 * i + 1)) for i in range(4)) + "\n")
    rng = ["-pk", "%x" % (1 << 40), "-pke", "%x" % ((1 << 41) - 1)]
    r = run(["-infile", str(keys), "-pb", compressed(mul(5))] + rng, tmp_path)
    assert r.returncode != 0 and "-pb and -infile" in r.stderr
    r = run(["-infile", str(keys), "-ksym"] + rng, tmp_path)
    assert r.returncode != 0 and "-ksym cannot be combined with -infile" in r.stderr
    r = run(["-infile", str(tmp_path / "missing.txt")] + rng, tmp_path)
    assert r.returncode != 0 and "open" in r.stderr
    r = run(["-infile", str(keys), "-wl", "nothing.work"] + rng, tmp_path)
    assert r.returncode != 0 and "cannot open" in r.stderr
    many = tmp_path / "many.txt"
    one = compressed(mul(3))
    many.write_text((one + "\n") * 65536)
    r = run(["-infile", str(many)] + rng, tmp_path)
    assert r.returncode != 0 and "65535" in r.stderr


def test_a_list_of_keys_at_the_start_of_the_range_needs_no_gpu(tmp_path):
    """every key equal to -pk: solved before any device is opened"""
    a = 1 << 40
    keys = tmp_path / "keys.txt"
    keys.write_text((compressed(mul(a)) + "\n") * 2)
    r = run(["-infile", str(keys), "-pk", "%x" % a, "-pke", "%x" % (2 * a - 1)], tmp_path)
    assert r.returncode == 0, r.stderr
    assert "Found 2 of 2" in r.stdout
    lines = (tmp_path / "win.txt").read_bytes().decode().split("\r\n")
    assert [l for l in lines if l.startswith("KEY[")] == ["KEY[1]: 0x%064x" % a, "KEY[2]: 0x%064x" % a]
