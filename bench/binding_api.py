"""The Python surface of the built _kernels extension, one line per public name, sorted.  CPU only.

usage: python bench/binding_api.py > api.txt

A callable prints its name and its whole pybind docstring (the typed signature, the keyword names
and defaults, the help text); anything else its name and repr.  Two builds bind the same interface
exactly when their outputs are byte-identical (diff them), as bench/isa_diff.py says of the kernels.
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    import torch  # noqa: F401  (the extension links against its libraries)
    from distributed_tensorflow_ibm_mnist_amd import _kernels as k
    for name in sorted(n for n in dir(k) if not n.startswith("_")):
        obj = getattr(k, name)
        print(name, repr(obj.__doc__) if callable(obj) else repr(obj))


if __name__ == "__main__":
    main()
