"""The recorded workspace sizes under tests/golden/ and the message counts they are recorded at: 1 and 2, both
sides of every plan block the entries use (410, 513, 1,025, 2,049), 65,536 and 2^20."""
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
M_VALUES = [1, 2, 409, 410, 512, 513, 1024, 1025, 2048, 2049, 65536, 1 << 20]


def recorded(name: str):
    """tests/golden/<name>.json: {argument(s): bytes}, or {function: {argument(s): bytes}}."""
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        return json.load(f)
