"""The one-pass FASTQ front end tests a dword for EOL bytes with a table lookup and packs four bases with a table lookup and a
dot product (kmerind_amd/csrc/kmi_front_bytes.h). tests/cpu/front_bytes_check.cpp runs those functions on the host, with the
header's host definitions of the two instructions, against byte-by-byte definitions: every pair of byte values in every pair of
positions of a dword, and 2e8 random dwords."""
import os
import subprocess


def test_front_byte_functions_match_bytewise_definitions(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "front_bytes_check")
    subprocess.check_call(["gcc", "-O2", "-x", "c++", "-I", os.path.join(root, "kmerind_amd", "csrc"),
                           os.path.join(root, "tests", "cpu", "front_bytes_check.cpp"), "-o", exe])
    out = subprocess.check_output([exe], text=True)
    assert out.startswith("front_bytes_check: ") and out.rstrip().endswith(" 0 mismatches"), out
