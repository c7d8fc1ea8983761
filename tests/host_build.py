"""Compiles a source under tests/host_shim/ with g++ -std=c++17: the product's headers built for the host as a shared library
that a test loads, or a stand-alone driver that a test runs.  Plain helper of the CPU tests; every caller names its own flags."""
import ctypes
import os
import subprocess

HOST_SHIM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_shim")
SHARED = ("-shared", "-fPIC")


def build(src, out, *flags):
    """g++ -std=c++17 <flags> -o <out> tests/host_shim/<src> -> out as a string"""
    subprocess.check_call(["g++", "-std=c++17", *flags, "-o", str(out), os.path.join(HOST_SHIM, src)])
    return str(out)


def load(path):
    return ctypes.CDLL(path)
