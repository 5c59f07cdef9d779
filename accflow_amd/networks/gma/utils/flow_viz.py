from ...raft.utils.flow_viz import flow_to_image  # noqa: F401
