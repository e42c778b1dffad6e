"""graph_weather/models/gencast/graph of the reference."""
