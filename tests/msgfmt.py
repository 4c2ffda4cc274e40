"""MF: oracle/message_format.py, loaded once. Every test, oracle and builder takes the message-format oracle
from here, so there is one module object and one NotEncodable / PropsParseError class in a test run."""
import importlib.util
import os

_spec = importlib.util.spec_from_file_location(
    "message_format", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle",
                                   "message_format.py"))
MF = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MF)
