#!/usr/bin/env python3
"""Fixture generator: the materials of the reference's only in-tree asset (resources/cornell.gltf), as data.  Run where a
checkout of the reference is at hand (the tests read only the fixture):

    python tests/golden/make_cornell_materials.py <reference checkout>/resources/cornell.gltf

Writes tests/golden/cornell_materials.json: the baseColorFactor of every material and the material index of every
primitive, in the order of tests/golden/cornell_scene.npz's instances (one per primitive of the mesh node)."""
import json
import os
import sys


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    with open(sys.argv[1]) as f:
        g = json.load(f)
    out = {"baseColorFactor": [m["pbrMetallicRoughness"]["baseColorFactor"] for m in g["materials"]],
           "primitiveMaterial": [p["material"] for n in g["nodes"] if "mesh" in n for p in g["meshes"][n["mesh"]]["primitives"]]}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cornell_materials.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(path)


if __name__ == "__main__":
    main()
