"""CPU: -kwalk at the command line of bsgs_mi355x -kangaroo, before any device is looked for: its values, what it may be combined with, and a list whose
keys all sit in the middle of the range, which the symmetric list search solves without a GPU."""
import os
import subprocess

from pybsgs.ecpy import mul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "bsgs-cuda_amd", "build", "bsgs_mi355x")
A = 1 << 40
RNG = ["-pk", "%x" % A, "-pke", "%x" % (2 * A - 1)]


def compressed(p):
    return "%02x%064x" % (2 + (p[1] & 1), p[0])


def run(args, cwd):
    if not os.path.exists(HOST):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "bsgs-cuda_amd"), "-s"])
    return subprocess.run([HOST, "-kangaroo", "-dir", str(cwd)] + args, capture_output=True, text=True, timeout=120)


def test_kwalk_parsing(tmp_path):
    keys = tmp_path / "keys.txt"
    keys.write_text("\n".join(compressed(mul(A + 7 * i + 1)) for i in range(4)) + "\n")
    one = compressed(mul(A + 5))
    r = run(["-infile", str(keys), "-kwalk", "fast"] + RNG, tmp_path)
    assert r.returncode != 0 and "-kwalk must be plain or sym" in r.stderr
    r = run(["-infile", str(keys), "-kwalk"], tmp_path)
    assert r.returncode != 0 and "missing value" in r.stderr
    # -ksym stays the flag of one key, with -kwalk sym beside it as well; the message names the way
    for extra in (["-ksym"], ["-ksym", "-kwalk", "sym"]):
        r = run(["-infile", str(keys)] + extra + RNG, tmp_path)
        assert r.returncode != 0 and "-ksym cannot be combined with -infile" in r.stderr and "-kwalk sym" in r.stderr
    # -kjumps and -kjumpscale belong to the symmetric walk, of one key or of a list
    for walk in ([], ["-kwalk", "plain"]):
        r = run(["-infile", str(keys), "-kjumps", "512"] + walk + RNG, tmp_path)
        assert r.returncode != 0 and "belong to -ksym" in r.stderr
        r = run(["-pb", one, "-kjumpscale", "2"] + walk + RNG, tmp_path)
        assert r.returncode != 0 and "belong to -ksym" in r.stderr
    # accepted: the run gets as far as its work file (read before any device is looked for)
    for args in (["-infile", str(keys), "-kwalk", "sym", "-kjumps", "512", "-kjumpscale", "1.5"], ["-pb", one, "-kwalk", "sym", "-kjumps", "512"],
                 ["-infile", str(keys), "-kwalk", "plain"], ["-pb", one, "-kwalk", "plain"]):
        r = run(args + ["-wl", "nothing.work"] + RNG, tmp_path)
        assert r.returncode != 0 and "cannot open" in r.stderr, r.stderr
    r = run(["-infile", str(keys), "-kwalk", "sym", "-pb", one] + RNG, tmp_path)
    assert r.returncode != 0 and "-pb and -infile" in r.stderr


def test_a_list_of_keys_in_the_middle_of_the_range_needs_no_gpu(tmp_path):
    keys = tmp_path / "keys.txt"
    keys.write_text((compressed(mul(A + A // 2)) + "\n") * 2)
    r = run(["-infile", str(keys), "-kwalk", "sym"] + RNG, tmp_path)
    assert r.returncode == 0, r.stderr
    assert "Found 2 of 2" in r.stdout
    lines = (tmp_path / "win.txt").read_bytes().decode().split("\r\n")
    assert [l for l in lines if l.startswith("KEY[")] == ["KEY[1]: 0x%064x" % (A + A // 2), "KEY[2]: 0x%064x" % (A + A // 2)]
